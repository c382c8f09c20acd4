"""The SKY blocks of a camera (rvpt_packets.hip: sky_blocks) without a GPU: a 16 x 4 block inside the image is sky when no triangle's screen rectangle
(rvpt_camera_rects, the host form of camera_rects) holds it — the camera round's predicate rect_holds over every rectangle.  At the headline's default camera
a little over half of a 1920 x 1080 frame is sky: the work the batched launches no longer claim."""
import numpy as np

from _util import scene_by_name
from test_camera_rects import prepared_records


def sky_blocks(rects, W, H):
    """bool[by, bx] over the blocks that hold a pixel of the image: True = no rectangle (x0, x1, y0, y1) holds it."""
    bx, by = np.arange((W + 15) // 16), np.arange((H + 3) // 4)
    held = np.zeros((by.size, bx.size), bool)
    for x0, x1, y0, y1 in rects:
        held[(by >= y0) & (by <= y1), :] |= (bx >= x0) & (bx <= x1)
    return ~held


def test_sky_blocks_of_the_default_camera():
    from rvpt_amd import Camera, native
    tris, _, _ = scene_by_name("default")
    W, H = 1920, 1080
    cam = Camera(W / H)
    cam.translation, cam.rotation, cam.fov = np.array((0, 0, 0), float), np.array((0, 0, 0), float), 90.0
    rects = native.camera_rects(prepared_records(tris), cam.get_data(), W, H)
    sky = sky_blocks(rects, W, H)
    assert sky.size == 32400
    assert int(sky.sum()) == 17222  # 53.2 % of the frame's blocks
    # ... and at the benchmark camera of SURVEY §8(d), looking at the model from further back, nearly all of it
    cam.translation = np.array((0, 0.9, -2.5), float)
    assert sky_blocks(native.camera_rects(prepared_records(tris), cam.get_data(), W, H), W, H).mean() > 0.9
