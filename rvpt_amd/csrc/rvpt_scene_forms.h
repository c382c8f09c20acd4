// rvpt_scene_forms.h — which form of rvpt_hip_upload_scene a call is (include/rvpt_hip.h: the sentinel counts in `n_nodes`), decided in one place, and what each
// form does to the rest pose and to the binding afterwards.  Pure host arithmetic on the header's own macros: no HIP header, so rvpt_amd/host/host_scene_forms.cpp
// compiles it alone and tests/test_scene_forms_host.py holds it against a restatement in Python.  rvpt_scene.hip is the one user inside the library.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/rvpt_hip.h"

namespace rv {

enum class SceneForm : uint32_t { Upload, BuildLbvh, BuildPloc, BuildSah, Update, UpdateGuarded, UpdateSparse, Pose, PoseGuarded, BindSkin, Skin, SkinGuarded };
constexpr uint32_t kSceneFormCount = 12;

// One row per form, in the order of SceneForm.  The two `keeps` columns are the header's rules for a call that SUCCEEDED (tests/_scene_model.py states them in
// numpy); a call of any form that leaves the context without a scene drops both, whatever its row says.
struct SceneFormRow {
    const char *name;       // for host_scene_forms' output
    const char *report;     // the first words of a guarded form's sentences in rvpt_hip_last_error; NULL: the form is not guarded
    bool keeps_binding;     // the skin update's binding survives the call
    bool keeps_rest;        // the rest pose survives the call: the next pose or skin update takes no fresh snapshot
    bool guard_carries_rest;  // the form's guard takes the rest pose through its rebuild: into the caller's order by the old permutation, back by the new one
    bool guard_names_tree;  // "rebuilt (<word>)" names the tree the scene then holds — lbvh after a PLOC rebuild that fell back — and not the builder that ran
};
constexpr SceneFormRow kSceneFormRows[kSceneFormCount] = {
    {"upload", nullptr, false, false, false, false},
    {"build-lbvh", nullptr, false, false, false, false},
    {"build-ploc", nullptr, false, false, false, false},
    {"build-sah", nullptr, false, false, false, false},
    {"update", nullptr, true, false, false, false},
    {"update-guarded", "guarded update", true, false, false, false},
    {"update-sparse", nullptr, true, false, false, false},
    {"pose", nullptr, true, true, false, false},
    {"pose-guarded", "guarded pose update", true, true, true, true},
    {"bind-skin", nullptr, true, true, false, false},
    {"skin", nullptr, true, true, false, false},
    {"skin-guarded", "guarded skin update", true, true, true, true},
};
constexpr const SceneFormRow &scene_form_row(SceneForm form) { return kSceneFormRows[static_cast<uint32_t>(form)]; }

struct SceneCall {
    SceneForm form;
    uint32_t permille;  // the limit a guarded count carries, 0 for every other form
    bool limit_ok;      // 0 (report only) or 1000 .. 65535; true for every other form
};

// a guarded band holds the permilles 0 .. kBandLast: `first` is the band's macro at 0, the counts run DOWN from there
constexpr uint32_t kBandLast = 0xFFFFFu;
constexpr bool in_band(size_t n_nodes, size_t first, size_t last) { return n_nodes <= first && n_nodes >= last; }
constexpr SceneCall guarded_call(SceneForm form, size_t n_nodes, size_t first)
{
    const uint32_t permille = static_cast<uint32_t>(first - n_nodes);
    return {form, permille, permille == 0 || (permille >= 1000u && permille <= 65535u)};
}

// The precedence is rvpt_hip_upload_scene's as it grew: the pose, bind and skin counts and the two guarded bands above them are forms WHATEVER `nodes`, `tris` and
// `mats` are (each refuses those itself, in its own words and order), and so is the sparse count; the update pattern is exact — triangles and nothing else —;
// the plain guarded band and the three build counts are forms only without a node array, and with one the call is an ordinary upload, which then validates
// the count as a node count.
constexpr SceneCall classify_scene_call(bool has_nodes, size_t n_nodes, bool has_tris, size_t n_tris, bool has_mats, size_t n_mats)
{
    if (n_nodes == RVPT_HIP_NODES_UPDATE_POSE) return {SceneForm::Pose, 0, true};
    if (n_nodes == RVPT_HIP_NODES_BIND_SKIN) return {SceneForm::BindSkin, 0, true};
    if (n_nodes == RVPT_HIP_NODES_UPDATE_SKIN) return {SceneForm::Skin, 0, true};
    if (in_band(n_nodes, RVPT_HIP_NODES_UPDATE_POSE_GUARDED(0), RVPT_HIP_NODES_UPDATE_POSE_GUARDED(kBandLast)))
        return guarded_call(SceneForm::PoseGuarded, n_nodes, RVPT_HIP_NODES_UPDATE_POSE_GUARDED(0));
    if (in_band(n_nodes, RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(0), RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(kBandLast)))
        return guarded_call(SceneForm::SkinGuarded, n_nodes, RVPT_HIP_NODES_UPDATE_SKIN_GUARDED(0));
    if (n_nodes == RVPT_HIP_NODES_UPDATE_SPARSE) return {SceneForm::UpdateSparse, 0, true};
    if (has_tris && n_tris > 0 && !has_nodes && n_nodes == 0 && !has_mats && n_mats == 0) return {SceneForm::Update, 0, true};
    if (!has_nodes && in_band(n_nodes, RVPT_HIP_NODES_UPDATE_GUARDED(0), RVPT_HIP_NODES_UPDATE_GUARDED(kBandLast)))
        return guarded_call(SceneForm::UpdateGuarded, n_nodes, RVPT_HIP_NODES_UPDATE_GUARDED(0));
    if (!has_nodes && n_nodes == RVPT_HIP_NODES_BUILD) return {SceneForm::BuildLbvh, 0, true};
    if (!has_nodes && n_nodes == RVPT_HIP_NODES_BUILD_PLOC) return {SceneForm::BuildPloc, 0, true};
    if (!has_nodes && n_nodes == RVPT_HIP_NODES_BUILD_SAH) return {SceneForm::BuildSah, 0, true};
    return {SceneForm::Upload, 0, true};
}

}  // namespace rv
