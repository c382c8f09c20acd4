// bvh_wide.h — the 4-wide regrouping of a binary BVH (bvh_wide.cpp), shared by the full upload (rvpt_scene.hip) and the exported rvpt_bvh_wide_form.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/rvpt_hip.h"

namespace rv {

constexpr uint32_t kWideFormChildren = 4;           // == kWideChildren (rvpt_kernels.h)
constexpr uint32_t kWideFormEmpty = 0xFFFFFFFFu;    // == kWideEmpty: head word of an unused child slot

// 32 floats (8 quads: minx[4] maxx[4] miny[4] maxy[4] minz[4] maxz[4] head[4] pad) per wide node, breadth first; empty when the tree has no
// wide form.  stack_need = the most slots a depth-first walk can hold at once.  kid_map (optional): 4 words per wide node, the index in `nodes` of the binary node
// whose box each child slot copies, kWideFormEmpty for an unused slot — what a geometry update needs to refresh the copies (rvpt_refit.hip: refit_wide_gather).
std::vector<float> build_wide_nodes(const rvpt_bvh_node *nodes, size_t n_nodes, uint32_t head_shift, uint32_t &stack_need, std::vector<uint32_t> *kid_map = nullptr);

}  // namespace rv
