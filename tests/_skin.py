"""A small weight generator for the skin update's tests: bones are centres spread along the scene's diagonal; each vertex takes the four nearest, weighted by
inverse square distance and normalised in double, then rounded to float32 (with fewer than four bones the spare influences have weight 0 on bone 0); the matrices
are a different small rotation about each centre plus a small offset.  Weights depend on the vertex position alone, so welded vertices stay welded."""
import numpy as np

from rvpt_amd import scene


def centres(tris, k):
    p = np.asarray(tris, dtype=np.float32).reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64)
    lo, hi = p.min(axis=0), p.max(axis=0)
    s = (np.arange(k, dtype=np.float64) + 0.5) / k
    return lo + s[:, None] * (hi - lo)


def weights(tris, k):
    """VERTEX_SKIN_DTYPE[3 n] for float32[n, 16] triangles and k bones"""
    p = np.asarray(tris, dtype=np.float32).reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64)
    c = centres(tris, k)
    d2 = ((p[:, None, :] - c[None, :, :]) ** 2).sum(axis=2) + 1e-6  # [3 n, k]
    take = min(4, k)
    near = np.argsort(d2, axis=1, kind="stable")[:, :take]
    w = 1.0 / np.take_along_axis(d2, near, axis=1)
    w = w / w.sum(axis=1, keepdims=True)
    rec = np.zeros(p.shape[0], dtype=scene.VERTEX_SKIN_DTYPE)
    rec["bone"][:, :take] = near
    rec["weight"][:, :take] = w.astype(np.float32)
    return rec


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


def bones(tris, k, phase=0.0):
    """float32[k, 3, 4]: x -> R_b (x - c_b) + c_b + t_b, a rotation of a few degrees about an axis of its own and an offset of a few percent of the extent"""
    c = centres(tris, k)
    p = np.asarray(tris, dtype=np.float32).reshape(-1, 4, 4)[:, :3, :3].reshape(-1, 3).astype(np.float64)
    ext = float(np.ptp(p, axis=0).max()) or 1.0
    out = np.zeros((k, 3, 4), dtype=np.float32)
    for b in range(k):
        a = 0.37 * b + phase
        rot = rotation((np.sin(a) + 0.2, 1.0, np.cos(1.7 * a)), 0.05 + 0.04 * np.sin(2.3 * a + 1.0))
        off = 0.03 * ext * np.array([np.sin(1.1 * a + 0.3), np.cos(0.7 * a) + 1.5, np.sin(1.9 * a + 2.0)])
        out[b, :, :3] = rot
        out[b, :, 3] = c[b] - rot @ c[b] + off
    return out


def no_minus_zero(tris) -> bool:
    v = np.ascontiguousarray(np.asarray(tris, dtype=np.float32).reshape(-1, 4, 4)[:, :3, :3])
    return not (v.view(np.uint32) == 0x80000000).any()
