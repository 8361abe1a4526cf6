// What restir_gi.hip and restir_gi_path.hip share: the parameters of ReSTIR GI's kernels and how k_restir_gi_initial_path, the initial
// pass of a stage with bounces > 1 (restir_gi.h `path`), gets the three it takes besides.  That kernel is a translation unit of its own,
// and repeats the front half of k_restir_gi_initial instead of sharing a body with it, so that the one-bounce kernels stay the code they
// were: the inliner weighs a function by its callers in the unit - one more kernel instance in restir_gi.hip changed the code of every
// kernel there, the temporal and the spatial ones included - and a body shared through a function changed k_restir_gi_initial's
// register allocation.
#pragma once
#include "restir_gi.h"

namespace tr {

constexpr int KB = TR_BLOCK;

struct RestirGiParams {
    float search_radius, max_confidence, min_ray_dist;
    float prob_point, prob_tri, prob_dir, prob_env;
    uint rng_seed, frame;              // pcg(rng_seed) or 0; the stage's frame counter
    int has_history;
    RestirSurface* surface;            // this frame's half
    const RestirSurface* prev_surface; // the other half
    RestirGiReservoir* canonical;
    RestirGiReservoir* history;
    RestirGiReproject* reproject;      // null without temporal reuse
    const f4* in;                      // null: (0, 0, 0, 1)
    f4* out;
    RestirGiInitialRecord* rec_initial;         // null unless options.record, as the five below
    RestirSurface* rec_secondary;
    RestirCandidateRecord* rec_light;
    RestirTemporalRecord* rec_temporal;
    RestirSpatialRecord* rec_spatial;
    RestirFinalRecord* rec_final;
};

// What k_restir_gi_initial_path takes besides: its loop count and its two records.  RestirGiParams stays as it is - a field more moves
// the kernel arguments of every kernel of the file and with them their code, the one-bounce kernels' included -
// so the three travel, in the initial pass of a stage with bounces > 1 only, in fields that pass does not read: has_history, rec_spatial
// and rec_final (the temporal and the spatial pass get those fields as ever).
struct RestirGiPathArgs {
    uint bounces;                               // 2 .. RESTIR_GI_MAX_BOUNCES
    RestirGiPathRecord* rec;                    // [pixel][bounces - 1]; null unless options.record, as the one below
    RestirSurface* surface;
};
inline void restir_gi_set_path_args(RestirGiParams& P, const RestirGiPathArgs& a) {
    P.has_history = (int)a.bounces; P.rec_spatial = (RestirSpatialRecord*)a.rec; P.rec_final = (RestirFinalRecord*)a.surface;
}
TR_DEV RestirGiPathArgs restir_gi_path_args(const RestirGiParams& P) {
    return {(uint)P.has_history, (RestirGiPathRecord*)P.rec_spatial, (RestirSurface*)P.rec_final};
}

using RestirGiKernel = void (*)(SceneView, LaunchCtx, int, ViewportList, RestirGiParams, uint*);
RestirGiKernel restir_gi_initial_path_kernel(bool two_level);      // restir_gi_path.hip

}  // namespace tr
