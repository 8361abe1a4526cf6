// k_restir_gi_initial_path for gfx950: the initial pass of a ReSTIR GI stage with bounces > 1 (restir_gi.h `path`), which restir_gi.hip
// launches in k_restir_gi_initial's place.  IEEE fp32 without contraction in a fixed order, no atomics, the same LDS stack rows for every
// traversal of a lane, one after the other.
#include "restir_gi_path.h"

namespace tr {
namespace {

using Kind = RestirGiKind;

TR_DEV bool finite3(f3 v) { return !(isnan(v.x) || isnan(v.y) || isnan(v.z) || isinf(v.x) || isinf(v.y) || isinf(v.z)); }

// The light sample of a path vertex: one draw, sample_canonical at the vertex, its contribution there and its shadow ray;
// (contribution * visibility) / light_pdf, non-finite -> 0.  `rnd` and `lrec` receive what the decision records keep.
template <bool TWO_LEVEL>
TR_DEV f3 restir_gi_light_sample(const SceneView& sv, const RestirGiParams& P, LocalSampler& ls, const RestirDomain& at, int* stack, int& overflow, u4& rnd,
                                 RestirCandidateRecord& lrec) {
    rnd = pcg4d(ls.rs);
    RestirLightRecord Lr;
    float light_pdf;
    const RestirSample s = restir_sample_canonical(sv, P, rnd, at.pos, Lr, light_pdf);
    f3 light_dir, light_norm;
    float light_dist2;
    const f3 contrib = restir_contribution(sv, s, Lr, at, light_dir, light_dist2, light_norm);
    const float visibility = restir_shadow<TWO_LEVEL>(sv, P.min_ray_dist, at.pos, contrib, light_dir, light_dist2, stack, overflow);
    f3 nee = (contrib * visibility) / light_pdf;
    if (!finite3(nee)) nee = F3(0.0f);
    lrec.light = s.type << 30 | s.index; lrec.light_data = s.data; lrec.pdf = light_pdf; lrec.contribution = contrib; lrec.visibility = visibility;
    return nee;
}

TR_DEV void restir_gi_write_path(RestirGiPathRecord* rec, RestirSurface* surface, const RestirGiPathRecord& p, const RestirDomain& at) {
    restir_set_word(rec, 0, u4{TR_U(p.draw.x), TR_U(p.draw.y), TR_U(p.pdf), p.traced});
    restir_set_word(rec, 1, u4{TR_U(p.dir.x), TR_U(p.dir.y), TR_U(p.dir.z), TR_U(p.t)});
    restir_set_word(rec, 2, u4{(uint)p.instance_id, (uint)p.primitive_id, TR_U(p.u), TR_U(p.v)});
    restir_set_word(rec, 3, p.light_draw);
    restir_set_word(rec, 4, u4{p.light, TR_U(p.light_data.x), TR_U(p.light_data.y), TR_U(p.light_pdf)});
    restir_set_word(rec, 5, u4{TR_U(p.contribution.x), TR_U(p.contribution.y), TR_U(p.contribution.z), TR_U(p.visibility)});
    restir_set_word(rec, 6, u4{TR_U(p.factor.x), TR_U(p.factor.y), TR_U(p.factor.z), 0u});
    restir_set_word(rec, 7, u4{TR_U(p.throughput.x), TR_U(p.throughput.y), TR_U(p.throughput.z), 0u});
    restir_set_word(rec, 8, u4{TR_U(p.L_o.x), TR_U(p.L_o.y), TR_U(p.L_o.z), 0u});
    restir_store_surface(surface, at, p.instance_id >= 0 ? p.instance_id : -1);
}

TR_DEV RestirGiPathRecord restir_gi_no_vertex() {
    RestirGiPathRecord p = {};
    p.instance_id = -1; p.primitive_id = -1; p.t = -1.0f; p.light = RESTIR_NULL_INDEX;
    return p;
}

// tile_pixel's launch shape (first_hit.h), the bound and the LDS rows of k_restir_gi_initial, whose front half this repeats up to the light
// sample at x_s (restir_gi_path.h says why).  What is final there - the surface record, the reprojection, the first four words of the
// initial record, x_s's record and its light sample - is written ahead of the walk, so that the walk does not carry it: across an
// iteration live are the vertex's RestirDomain, T, L_o and the sampler, next to what the tail needs of the pixel (its RestirDomain and
// pdf) and of x_s (position and normal).  The loop count is the launch's; a lane that has ended (or never began) is masked and writes
// the records of a vertex not reached; a wave leaves the loop when none of its lanes is alive, and fills the records left.
template <bool TWO_LEVEL>
__global__ __launch_bounds__(KB, 2) void k_restir_gi_initial_path(SceneView sv, LaunchCtx L, int projection, ViewportList list, RestirGiParams P, uint* overflow_flag) {
    __shared__ int s_stack_rows[TR_STACK_WORDS];
    int* const s_stack = s_stack_rows + TR_STACK_ROW0;
    int px, py;
    tile_pixel(px, py);
    if ((uint)px >= L.launch_w || (uint)py >= L.launch_h) return;
    const RestirGiPathArgs A = restir_gi_path_args(P);
    const uint layer = blockIdx.z, viewport = list.v[layer];
    const CameraData cam = sv.cameras[viewport];
    f3 ray_origin, dir;
    HitRecord hit;
    int overflow;
    first_hit<TWO_LEVEL>(sv, L, cam, projection, px, py, P.min_ray_dist, s_stack + threadIdx.x, ray_origin, dir, hit, overflow);
    const size_t layer_px = (size_t)L.launch_w * L.launch_h;
    const size_t pix = layer * layer_px + (size_t)py * L.launch_w + (uint)px;
    RestirDomain dom = {}, at = {};                // the pixel's surface; the walk's vertex, x_s first
    LocalSampler ls = {};
    float pdf = 0.0f;
    f3 L_o = F3(0.0f);
    bool alive = false;
    {
        RestirGiInitialRecord irec = {};
        irec.instance_id = -1; irec.primitive_id = -1; irec.t = -1.0f;
        RestirCandidateRecord lrec = {};
        lrec.light = RESTIR_NULL_INDEX;
        HitRecord hit2;
        hit2.instance_id = -1;
        f2 motion = F2(0.0f);
        float origin_dist = 0.0f;
        if (hit.instance_id >= 0) {
            SurfacePoint v;
            first_hit_surface(sv, hit, dir, ray_origin, v, dom.mat);
            dom.pos = v.pos; dom.mapped_normal = v.mapped_normal; dom.flat_normal = v.hard_normal;
            dom.view = normalize(v.pos - ray_origin);
            if (P.reproject) {       // get_reprojected_pixel before its rounding (restir_di.h `reprojection`)
                const f3 prev_pos = surface_prev_pos(sv, hit.instance_id, hit.primitive_id, hit.u, hit.v);
                const f3 m = get_camera_projection(sv.prev_cameras[viewport], projection, prev_pos);
                motion = F2(m.x, 1.0f - m.y) * F2((float)L.launch_w, (float)L.launch_h) - 0.5f;
                origin_dist = length(ray_origin - dom.pos);
            }
            ls = init_local_sampler(u4{(uint)px, (uint)py, viewport, RESTIR_GI_SAMPLER_W}, 3u * P.frame, P.rng_seed, SAMPLER_UNIFORM);
            const f4 u = u4_to_unit(pcg4d(ls.rs));
            const f3 local = sample_cosine_hemisphere<RoundedMath>(F2(u.x, u.y));
            const f3 out_dir = mul(create_tangent_space(dom.mapped_normal), local);
            pdf = pdf_cosine_hemisphere(local);
            const bool cast = !(dot(out_dir, dom.flat_normal) < 1e-6f || pdf <= 0.0f);
            irec.draw = F2(u.x, u.y); irec.pdf = pdf; irec.traced = cast ? 1u : 0u; irec.dir = out_dir;
            if (cast) {
                TraceStats st = {};
                trace_closest4<1, false, TWO_LEVEL>(sv, dom.pos, out_dir, P.min_ray_dist, __builtin_huge_valf(), 0u, s_stack + threadIdx.x, hit2, st, overflow);
            }
            if (hit2.instance_id >= 0) {
                irec.instance_id = hit2.instance_id; irec.primitive_id = hit2.primitive_id; irec.u = hit2.u; irec.v = hit2.v; irec.t = hit2.t;
                SurfacePoint v2;
                first_hit_surface(sv, hit2, out_dir, dom.pos, v2, at.mat);
                at.pos = v2.pos; at.mapped_normal = v2.mapped_normal; at.flat_normal = v2.hard_normal;
                at.view = normalize(v2.pos - dom.pos);
                L_o = restir_gi_light_sample<TWO_LEVEL>(sv, P, ls, at, s_stack + threadIdx.x, overflow, irec.light_draw, lrec);      // NEE_1
                alive = true;
            }
        }
        restir_store_surface(P.surface + pix, dom, hit.instance_id >= 0 ? hit.instance_id : -1);
        if (P.reproject) restir_set_word(P.reproject + pix, 0, u4{TR_U(motion.x), TR_U(motion.y), TR_U(origin_dist), 0u});
        if (P.rec_initial) {
            RestirGiInitialRecord* rec = P.rec_initial + pix;
            restir_set_word(rec, 0, u4{TR_U(irec.draw.x), TR_U(irec.draw.y), TR_U(irec.pdf), irec.traced});
            restir_set_word(rec, 1, u4{TR_U(irec.dir.x), TR_U(irec.dir.y), TR_U(irec.dir.z), TR_U(irec.t)});
            restir_set_word(rec, 2, u4{(uint)irec.instance_id, (uint)irec.primitive_id, TR_U(irec.u), TR_U(irec.v)});
            restir_set_word(rec, 3, irec.light_draw);
            restir_store_surface(P.rec_secondary + pix, at, hit2.instance_id >= 0 ? hit2.instance_id : -1);
            RestirCandidateRecord* lr = P.rec_light + pix;
            restir_set_word(lr, 0, u4{lrec.light, TR_U(lrec.light_data.x), TR_U(lrec.light_data.y), TR_U(lrec.pdf)});
            restir_set_word(lr, 1, u4{TR_U(lrec.contribution.x), TR_U(lrec.contribution.y), TR_U(lrec.contribution.z), TR_U(lrec.visibility)});
            restir_set_word(lr, 2, u4{0u, 0u, 0u, 0u});
        }
    }
    const f3 x_s = at.pos, n_s = at.flat_normal;
    f3 T = F3(1.0f);
    uint k = 1u;
#pragma unroll 1
    for (; k < A.bounces; ++k) {
        if (__ballot(alive) == 0ull) break;
        RestirGiPathRecord prec = restir_gi_no_vertex();
        RestirDomain next = {};
        if (alive) {
            alive = false;
            const f4 u = u4_to_unit(pcg4d(ls.rs));
            const f3 local = sample_cosine_hemisphere<RoundedMath>(F2(u.x, u.y));
            const f3 out_dir = mul(create_tangent_space(at.mapped_normal), local);
            const float pdf_k = pdf_cosine_hemisphere(local);
            const bool cast = !(dot(out_dir, at.flat_normal) < 1e-6f || pdf_k <= 0.0f);
            prec.draw = F2(u.x, u.y); prec.pdf = pdf_k; prec.traced = cast ? 1u : 0u; prec.dir = out_dir;
            HitRecord hk;
            hk.instance_id = -1;
            if (cast) {
                TraceStats st = {};
                trace_closest4<1, false, TWO_LEVEL>(sv, at.pos, out_dir, P.min_ray_dist, __builtin_huge_valf(), 0u, s_stack + threadIdx.x, hk, st, overflow);
            }
            if (hk.instance_id >= 0) {
                prec.instance_id = hk.instance_id; prec.primitive_id = hk.primitive_id; prec.u = hk.u; prec.v = hk.v; prec.t = hk.t;
                SurfacePoint vk;
                first_hit_surface(sv, hk, out_dir, at.pos, vk, next.mat);
                next.pos = vk.pos; next.mapped_normal = vk.mapped_normal; next.flat_normal = vk.hard_normal;
                next.view = normalize(vk.pos - at.pos);
                Kind::Eval e;
                const f3 factor = Kind::contribution(sv, RestirGiSample{next.pos, next.flat_normal, F3(1.0f)}, at, e) / pdf_k;
                T = T * factor;
                prec.factor = factor; prec.throughput = T;
                at = next;
                if (finite3(T) && restir_casts(T)) {
                    RestirCandidateRecord lk = {};
                    const f3 nee = restir_gi_light_sample<TWO_LEVEL>(sv, P, ls, at, s_stack + threadIdx.x, overflow, prec.light_draw, lk);
                    prec.light = lk.light; prec.light_data = lk.light_data; prec.light_pdf = lk.pdf; prec.contribution = lk.contribution; prec.visibility = lk.visibility;
                    L_o = L_o + T * nee;
                    alive = true;
                }
            }
            prec.L_o = L_o;
        }
        if (A.rec) {
            const size_t slot = pix * (A.bounces - 1u) + (k - 1u);
            restir_gi_write_path(A.rec + slot, A.surface + slot, prec, next);
        }
    }
    if (A.rec) {             // the vertices no lane of the wave reached
        const RestirGiPathRecord none = restir_gi_no_vertex();
        const RestirDomain nowhere = {};
#pragma unroll 1
        for (; k < A.bounces; ++k) {
            const size_t slot = pix * (A.bounces - 1u) + (k - 1u);
            restir_gi_write_path(A.rec + slot, A.surface + slot, none, nowhere);
        }
    }
    if (overflow) *overflow_flag = 1;
    Kind::State r = Kind::create();                // the initial sample; uc_weight holds its pdf until the temporal kernel
    r.uc_weight = 1.0f;
    if (restir_casts(L_o)) {                       // the null sample otherwise; L_o is 0 where there was no x_s
        r.s.x = x_s; r.s.n = n_s; r.s.L = L_o;
        r.uc_weight = pdf;
        Kind::Eval e;
        r.target_function = rgb_to_luminance(Kind::contribution(sv, r.s, dom, e));
    }
    Kind::store(P.canonical + pix, r);
    if (P.rec_initial) restir_set_word(P.rec_initial + pix, 4, u4{TR_U(L_o.x), TR_U(L_o.y), TR_U(L_o.z), TR_U(r.target_function)});
}

}  // namespace

RestirGiKernel restir_gi_initial_path_kernel(bool two_level) { return two_level ? k_restir_gi_initial_path<true> : k_restir_gi_initial_path<false>; }

}  // namespace tr
