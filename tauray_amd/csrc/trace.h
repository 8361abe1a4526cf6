// BVH traversal + watertight ray/triangle test for gfx950 (wave64).
//
// Replaces the Vulkan driver's traceRayEXT (shader/path_tracer.glsl:38-50,387-403)
// and the hit/miss shader table (shader/rt_common*.r*).  One ray per lane; each
// lane keeps its short traversal stack in LDS (column layout stack[entry][lane]
// -> conflict free for ds_read/write_b32 regardless of per-lane depth) and
// spills to a private array only past LDS_STACK entries.
#pragma once
#include "common.h"
#include "rng.h"
#include "texture.h"
#include "trace_timeline.h"

namespace tr {

#ifndef TR_BLOCK
#define TR_BLOCK 256
#endif
#ifndef TR_VOTE
#define TR_VOTE 32         // closest-hit traversal: lanes holding a leaf wait until this many do - or half of the live lanes, which
                           // with 32 is always the smaller number (0 disables the vote).  8 before the quad tail took over the
                           // thin end of a wave, 16 after it; re-measured on the static-build tree: 12 / 16 / 24 / 32 = 3.89 / 3.85 /
                           // 3.81 / 3.79 ms per frame, and 3 / 5 / 6 eighths of the live lanes instead of half: 3.84 / 3.84 / 3.88
#endif
#ifndef TR_VOTE_SHADOW_WAVE
#define TR_VOTE_SHADOW_WAVE 16   // the same vote in the per-lane loop of trace_shadow_wave4 (0: none); 8 / 16 measured: -1 ... -2 % shadow time
#endif
// The slab test compares a box's entry distance with min(exit distance, current closest hit / tmax) * TR_SLAB_PAD.  The pad
// covers the rounding of both slab distances and, on the tmax side, the error of the distance the triangle test computes
// (a different expression): without it a box can be culled against a hit that one of its own triangles would have beaten
// by a few ulps, and which of two nearly coincident surfaces wins then depends on the shape of the tree.
#ifndef TR_SLAB_PAD
#define TR_SLAB_PAD 1.000004f
#endif
#define TR_LDS_STACK 16
#ifndef TR_SPILL_STACK
#define TR_SPILL_STACK 112
#endif

// A ray as the traversal keeps it: in the frame the watertight triangle test works in - components in the order (kx, ky, kz), kz the axis
// the direction is largest along (Woop et al. 2013).  Round 5: the slab test does not care in which order it takes the axes (its
// near / far planes are picked by per-lane byte offsets anyway), and the triangle test picks the vertex components it wants with explicit
// selects on 4 kx / 4 ky / 4 kz (tri_intersect) - a component picked out of a vector by a run-time index is lowered to exec-mask branches:
// nine such picks per triangle test were 150 of its 335 instructions
// (profiles/r5/trace_phase_timeline.txt: a triangle phase spent 2 400 clocks there, twice a node phase's slab tests and sort).
struct RayPre {
    f3 op;                // origin in the order (kx, ky, kz)
    f3 ip;                // 1 / direction, same order
    float Sx, Sy;         // shear constants of the triangle test; the third one, 1 / direction[kz], is ip.z
    uint nkx, nky, nkz;   // byte offsets of the near planes of the axes kx / ky / kz inside a Bvh4Node: 32 k + 16 (direction[k] < 0); far plane: offset ^ 16
};
TR_DEV uint tri_component_offset(uint nk) { return (nk >> 3) & 12u; }     // 4 k: byte offset of component k of a vertex

TR_DEV RayPre make_ray(f3 org, f3 dir) {
    RayPre r;
    float ax = fabsf(dir.x), ay = fabsf(dir.y), az = fabsf(dir.z);
    int kz = (ax > ay) ? (ax > az ? 0 : 2) : (ay > az ? 1 : 2);
    int kx = kz + 1; if (kx == 3) kx = 0;
    int ky = kx + 1; if (ky == 3) ky = 0;
    if (comp(dir, kz) < 0.0f) { int t = kx; kx = ky; ky = t; }
    const float dkx = comp(dir, kx), dky = comp(dir, ky), dkz = comp(dir, kz);
    r.Sx = dkx / dkz;
    r.Sy = dky / dkz;
    r.op = F3(comp(org, kx), comp(org, ky), comp(org, kz));
    r.ip = F3(1.0f / dkx, 1.0f / dky, 1.0f / dkz);
    r.nkx = ((uint)kx << 5) | ((__float_as_uint(r.ip.x) >> 31) << 4);
    r.nky = ((uint)ky << 5) | ((__float_as_uint(r.ip.y) >> 31) << 4);
    r.nkz = ((uint)kz << 5) | ((__float_as_uint(r.ip.z) >> 31) << 4);
    return r;
}

TR_DEV bool ray_is_finite(f3 o, f3 d) {
    return isfinite(o.x) && isfinite(o.y) && isfinite(o.z) && isfinite(d.x) && isfinite(d.y) && isfinite(d.z) &&
           (d.x != 0.0f || d.y != 0.0f || d.z != 0.0f);
}

// A ray of the terminal query (trace_quad.h trace_closest_wave4<.., TERMINAL>).  `early`: the ray may end at the first accepted candidate
// that replaces its best so far (false: an ordinary closest hit, the per-ray fallback).  `blocked`: it did.
struct TerminalRay { bool early, blocked; };
// HitRecord::instance_id of a blocked ray in the output of k_query_terminal (a frame's blocked paths get no record at all)
#define TR_HIT_BLOCKED (-2)

// The per-ray fallback predicate.  A blocked path is dropped because its last k_shade pass would add exactly nothing: for a hit on a
// triangle that is not in the emitter set, mat.emission, every light term and every light pdf are zero, so
//     light = (attenuation / bsdf_pdf) * mis_weight * 0,      mis_weight = bsdf_pdf / ((0 * 0 + bsdf_pdf * bsdf_pdf) / bsdf_pdf)  (power heuristic)
// which is +-0 - and not written - exactly when the two factors are finite.  With 2^-40 <= bsdf_pdf <= 2^40 the square stays in
// [2^-80, 2^80] (no overflow to inf, no underflow to 0), mis_pdf is bsdf_pdf to a few ulps in either shading arithmetic and
// mis_weight is 1 to a few ulps (balance heuristic and no MIS: exactly bsdf_pdf, weight 1); with |attenuation| <= 2^40 per
// component the quotient is at most 2^80 (1 + a few ulps).  bsdf_pdf == 0 skips the division and the weight (mis_weight = 1), and
// the attenuation bound alone keeps the product finite.  The comparisons are false for NaN, so a NaN in either sends the ray down
// the fallback.  clamp_contribution_mul of a zero light returns 1.
TR_DEV bool terminal_early_ok(float bsdf_pdf, f3 attenuation) {
    const float lo = 9.094947017729282e-13f, hi = 1099511627776.0f;      // 2^-40, 2^40
    const bool pdf_ok = bsdf_pdf == 0.0f || (bsdf_pdf >= lo && bsdf_pdf <= hi);
    return pdf_ok && fabsf(attenuation.x) <= hi && fabsf(attenuation.y) <= hi && fabsf(attenuation.z) <= hi;
}

// What a triangle test hands back: the candidate and the words of the record behind the vertices.
struct TriHit { float t, bu, bv; uint inst_flags, prim, alpha; };

// Watertight test (Woop, Benthin, Wald 2013), no culling, of triangle record `index`.  Plain IEEE fp32 without
// contraction: the shared-edge guarantee needs both products of each edge function
// rounded, and the CPU oracle evaluates exactly the same expression tree.  The nine vertex components are taken in the ray's order.
TR_DEV bool tri_intersect(const RayPre& r, const TriRecord* tris, uint index, float tmin, float tmax, TriHit& o TL(, TlPhase* tlp = nullptr)) {
#pragma clang fp contract(off)
    // The record is three 16-byte loads - what a lane's L1 pays for is accesses, not bytes - and every component is picked out of the three
    // registers of its vertex with two selects (18 selects per test).  Round 5 measured both ways of not branching over the axes
    // (profiles/r5/triangle_fetch_ab.txt): nine 4-byte loads at per-lane offsets 4 kx / 4 ky / 4 kz cost no vector instruction at all and ten
    // L1 accesses instead of three; the selects win by 4 % of the closest-hit kernel - the vector L1 is the busiest unit of these kernels
    // (0.65 of its access rate), the VALUs are not (0.43).
    const f4* p = reinterpret_cast<const f4*>(reinterpret_cast<const char*>(tris) + (size_t)index * (uint)sizeof(TriRecord));
    const f4 q0 = p[0], q1 = p[1], q2 = p[2];       // x0 y0 z0 x1 | y1 z1 x2 y2 | z2 inst prim alpha
    // a caller that does not look at every word (the any-hit loops never read `prim`) would have the third load cut into the pieces it
    // does read: two accesses for one.  The asm makes the four words one value that is used where the vertices are
    float z2 = q2.x, w_inst = q2.y, w_prim = q2.z, w_alpha = q2.w;
    asm volatile("" : "+v"(z2), "+v"(w_inst), "+v"(w_prim), "+v"(w_alpha));
    o.inst_flags = __float_as_uint(w_inst); o.prim = __float_as_uint(w_prim); o.alpha = __float_as_uint(w_alpha);
    const uint kx4 = tri_component_offset(r.nkx), ky4 = tri_component_offset(r.nky), kz4 = tri_component_offset(r.nkz);
    auto pick = [](float x, float y, float z, uint k4) { const float xy = k4 == 4u ? y : x; return k4 == 8u ? z : xy; };
    const float v0x = pick(q0.x, q0.y, q0.z, kx4), v1x = pick(q0.w, q1.x, q1.y, kx4), v2x = pick(q1.z, q1.w, z2, kx4);
    const float v0y = pick(q0.x, q0.y, q0.z, ky4), v1y = pick(q0.w, q1.x, q1.y, ky4), v2y = pick(q1.z, q1.w, z2, ky4);
    const float v0z = pick(q0.x, q0.y, q0.z, kz4), v1z = pick(q0.w, q1.x, q1.y, kz4), v2z = pick(q1.z, q1.w, z2, kz4);
    TL(if (tlp) tlp->loads_issued();)
    const float Akz = v0z - r.op.z, Bkz = v1z - r.op.z, Ckz = v2z - r.op.z;
    const float Ax = (v0x - r.op.x) - r.Sx * Akz, Ay = (v0y - r.op.y) - r.Sy * Akz;
    const float Bx = (v1x - r.op.x) - r.Sx * Bkz, By = (v1y - r.op.y) - r.Sy * Bkz;
    const float Cx = (v2x - r.op.x) - r.Sx * Ckz, Cy = (v2y - r.op.y) - r.Sy * Ckz;
    float U = Cx * By - Cy * Bx;
    float V = Ax * Cy - Ay * Cx;
    float W = Bx * Ay - By * Ax;
    if (U == 0.0f || V == 0.0f || W == 0.0f) {
        double CxBy = (double)Cx * (double)By, CyBx = (double)Cy * (double)Bx;
        U = (float)(CxBy - CyBx);
        double AxCy = (double)Ax * (double)Cy, AyCx = (double)Ay * (double)Cx;
        V = (float)(AxCy - AyCx);
        double BxAy = (double)Bx * (double)Ay, ByAx = (double)By * (double)Ax;
        W = (float)(BxAy - ByAx);
    }
    if ((U < 0.0f || V < 0.0f || W < 0.0f) && (U > 0.0f || V > 0.0f || W > 0.0f)) return false;
    const float det = U + V + W;
    if (det == 0.0f) return false;
    const float Az = r.ip.z * Akz, Bz = r.ip.z * Bkz, Cz = r.ip.z * Ckz;
    const float T = U * Az + V * Bz + W * Cz;
    const float rcp = 1.0f / det;
    const float tt = T * rcp;
    if (!(tt > tmin && tt < tmax)) return false;
    o.t = tt; o.bu = V * rcp; o.bv = W * rcp;
    return true;
}

// Per-lane traversal stack: the top entry in a register, the next TR_LDS_STACK in LDS, the rest in a private spill array.
// `sp` must stay in a VGPR and the LDS access must stay a ds_read/ds_write: the spill array is therefore a separate
// local (a struct member array drags the whole struct, sp included, into scratch) and pop() reads LDS
// unconditionally, through a pointer typed as LDS (an if/else over the two memories through generic pointers is if-converted into a
// select of pointers + flat_load).
//
// Round 5 (profiles/r5/trace_phase_timeline.txt): a wave gets an instruction issued every 6-7 clocks at six waves per SIMD whatever
// its kind, and the three conditional pushes of a node phase + the pop were ~120 instructions and an LDS round trip - more clocks than
// the four slab tests and the sort.  Now: entry sp - 1 lives in `tos`, rows 0 .. sp - 2 in memory; a node phase stores the old top and
// up to two of the sorted children with three unconditional ds_writes (rows above the new top hold junk, which nothing reads), and a pop
// hands out the register and refills it with a ds_read whose result nothing in pop() uses.  Row -1 exists (the kernels
// allocate one row more and pass the address of row 0): the store of the "old top" of an empty stack lands there.
//
// Round 22, as compiled (profiles/r22/anyhit_stack.txt): both push forms are selects for the new top and depth, one
// ds_write2st64_b32 + one ds_write_b32, and the spill stores out of line behind one branch on the depth.  The pop's ds_read_b32 lands in
// the register of `tos` and is not waited for behind the read.  In the closest-hit loops the wait stands in front of the next push's
// store or the next pop; in the any-hit loops it stands at the head of the next iteration of the wave loop, where the compiler copies
// the loop's values (some twenty instructions behind the read).  It would take a loop the structuriser leaves alone to move that one too.
typedef __attribute__((address_space(3))) int lds_int;
struct LaneStack {
    int* lds;           // &stack[0][lane_in_block]; stride TR_BLOCK; row -1 is writable
    int sp;             // entries, the one in `tos` included
    int tos;
    bool overflow;      // a store was dropped (a lane mask in scalar registers: the per-lane counter this used to be held a vector register for nothing)
    TR_DEV void init(int* base) { lds = base; sp = 0; tos = 0; overflow = false; }
    // row r of the memory part (r >= -1).  Past the end of the spill array stores land on its last slot and are counted: the traversal
    // still terminates (sp stays balanced) and the frame is reported as invalid.
    TR_DEV void store_row(int* spill, int r, int v) {
        if (r < TR_LDS_STACK) lds[r * TR_BLOCK] = v;
        else {
            const int k = r - TR_LDS_STACK;
            if (k >= TR_SPILL_STACK) overflow = true;
            spill[k < TR_SPILL_STACK ? k : TR_SPILL_STACK - 1] = v;
        }
    }
    TR_DEV void push(int* spill, int v) {
        store_row(spill, sp - 1, tos);
        tos = v;
        sp++;
    }
    // The hit children of a node phase other than the one the ray descends into, nearest last: `m` of (c3, c2, c1) are valid - the last m.
    TR_DEV void push_sorted(int* spill, int m, int c1, int c2, int c3) {
        if (sp + 2 <= TR_LDS_STACK) {     // rows sp - 1, sp, sp + 1 are LDS rows
            int* row = lds + (sp - 1) * TR_BLOCK;
            row[0] = tos;
            row[TR_BLOCK] = m == 3 ? c3 : c2;
            row[2 * TR_BLOCK] = c2;
            tos = m > 0 ? c1 : tos;
            sp += m;
        } else {
            if (m > 2) push(spill, c3);
            if (m > 1) push(spill, c2);
            if (m > 0) push(spill, c1);
        }
    }
    // ... in slot order, for the any-hit loop (which descends into the first hit child and keeps the others in the order of their slots):
    // `n` hit children behind the first; the last of them is `top`, the first two are a and b
    TR_DEV void push_packed(int* spill, int n, int a, int b, int top) {
        // bottom to top: old top, a, b | top (n = 3);  old top, a | top = b (n = 2);  old top | top = a (n = 1).
        // The new top and depth are selects outside the branch on the depth, so that its two arms hold stores and nothing else: with
        // `tos` and `sp` assigned in both, the arms were merged and the three conditional stores of the deep one became a dozen
        // exec-mask blocks on the common path (profiles/r22/anyhit_stack.txt).
        const int old = tos, r0 = sp - 1;
        tos = n > 0 ? top : tos;
        sp += n;
        if (__builtin_expect(r0 + 2 < TR_LDS_STACK, 1)) {     // rows r0, r0 + 1, r0 + 2 are LDS rows
            int* row = lds + r0 * TR_BLOCK;
            row[0] = old;
            row[TR_BLOCK] = a;
            row[2 * TR_BLOCK] = b;
        } else {                // the rows a chain of n push() calls stores, each to its own memory
            if (n > 0) store_row(spill, r0, old);
            if (n > 1) store_row(spill, r0 + 1, a);
            if (n > 2) store_row(spill, r0 + 2, b);
        }
    }
    TR_DEV int pop(const int* spill) {
        int out = tos;
        asm volatile("" : "+v"(out));     // the old top leaves its register here, ahead of the read that refills it
        sp--;
        const int r = sp - 1;       // the row that becomes the top: -1 (junk, never handed out) when the stack is empty now
        // the column through a pointer that can only be LDS: the read stays a ds_read whatever is done with its result, and nothing
        // here uses the result - where the wait for it ends up: see above
        int v = ((const lds_int*)lds)[(r < TR_LDS_STACK ? r : 0) * TR_BLOCK];
        if (__builtin_expect(r >= TR_LDS_STACK, 0)) v = spill[r - TR_LDS_STACK < TR_SPILL_STACK ? r - TR_LDS_STACK : TR_SPILL_STACK - 1];
        tos = v;
        return out;
    }
    // every entry in memory (rows 0 .. sp - 1): what the re-deal to quads reads (trace_quad.h)
    TR_DEV void flush(int* spill) { store_row(spill, sp - 1, tos); }
};

struct TraceStats {
    uint nodes, tris, alpha, maxsp;
    // divergence statistics of the closest-hit loop (counting builds only), kept by the first active lane of a wave: node / triangle
    // phases executed, node phases that ran with at most 16 / 8 active rays, and the ray visits those phases served
    uint ph_node, ph_tri, ph_node16, ph_node8, lv_node16;
    uint ph_qnode, ph_qtri;   // phases of the quad-cooperative tail (trace_quad.h)
    uint ph_hist[8];          // per-lane node phases by live rays: 1-8, 9-16, ..., 57-64
    uint cnodes;              // node visits of closest-hit rays alone (`nodes` also counts the shadow rays of a fused launch)
    uint ltests, lnodes, lfallbacks;   // sphere-light tests, light-tree node visits, walks that fell back to the loop (trhip_pt_get_light_counters)
};

// Candidate alpha of a non-opaque triangle: albedo_factor.a * texture alpha at the uv of the candidate hit
// (get_interpolated_vertex_light, shader/rt.glsl:103-117; shader/rt_common.rahit:15-24).  `word` = TriRecord::alpha: the alpha itself for
// an untextured material, else the triangle's AlphaTri record - one 32-byte fetch where the instance, its span, three indices and three
// vertices used to be fetched one behind the other (same values, same expressions: common.h, bvh_build.hip alpha_word).
TR_DEV float candidate_alpha(const SceneView& sv, uint word, float bu, float bv) {
    if (!(word & 0x80000000u)) return __uint_as_float(word);
    // both 16-byte halves of the record are asked for together, ahead of the test of `tex`: left alone, the compiler fetches (factor, tex)
    // first and the uvs only behind that test, a second dependent round trip for every textured candidate
    const f4* p = reinterpret_cast<const f4*>(sv.alpha_tris + (word & 0x7FFFFFFFu));
    const f4 lo = p[0], hi = p[1];        // uv0 uv1 | uv2 factor tex
    float u0x = lo.x, u0y = lo.y, u1x = lo.z, u1y = lo.w, u2x = hi.x, u2y = hi.y, alpha = hi.z, texw = hi.w;
    asm volatile("" : "+v"(u0x), "+v"(u0y), "+v"(u1x), "+v"(u1y), "+v"(u2x), "+v"(u2y), "+v"(alpha), "+v"(texw));
    const int tex = __float_as_int(texw);
    if (tex >= 0) {
        const float b0 = 1.0f - bu - bv;
        alpha *= sample_texture_alpha(sv, tex, F2(u0x, u0y) * b0 + F2(u1x, u1y) * bu + F2(u2x, u2y) * bv);
    }
    return alpha;
}

// Traversal-order independent stand-in for generate_single_uniform_random(payload.random_seed)
// (shader/rt_common.rahit:21); see DESIGN.md "any-hit order".
TR_DEV float alpha_cutoff_hash(uint seed, int instance_id, int primitive_id) {
    uint k = (uint)instance_id * 0x9E3779B9u + (uint)primitive_id;
    uint h = seed ^ pcg(k);
    return (float)pcg(h) * 2.3283064365386963e-10f;
}

// =====================================================================================================================
// 4-wide fp32 BVH: half the dependent node fetches of the binary tree for about the same box-test arithmetic.
struct Hit4 { float t[4]; int c[4]; };

// The ray's direction signs pick the near and the far plane of every axis at load time (per-lane byte offsets into the
// 128-byte node), so the slab test needs no min / max to order them: per child 6 sub, 6 mul, max + max3, min3 + pad + min,
// one compare.  NaNs (0 * inf: origin on a plane of an axis the ray does not move along) are dropped by min / max, i.e.
// that axis does not constrain the interval.  Empty slots hold an inverted infinite box: their near distance is +inf (or
// their far distance -inf) for every ray, so they never pass and need no test of their own.
struct Node4Data { f4 nxv, fxv, nyv, fyv, nzv, fzv; int4 ch; };      // near / far planes of the axes kx, ky, kz and the child references
TR_DEV void box4_load(const RayPre& r, const Bvh4Node* nodes, int node, Node4Data& d) {
    const char* base = reinterpret_cast<const char*>(nodes);
    const uint t = (uint)node << 7;
    const uint ax = t | r.nkx, ay = t | r.nky, az = t | r.nkz;
    d.nxv = *reinterpret_cast<const f4*>(base + (size_t)ax); d.fxv = *reinterpret_cast<const f4*>(base + (size_t)(ax ^ 16u));
    d.nyv = *reinterpret_cast<const f4*>(base + (size_t)ay); d.fyv = *reinterpret_cast<const f4*>(base + (size_t)(ay ^ 16u));
    d.nzv = *reinterpret_cast<const f4*>(base + (size_t)az); d.fzv = *reinterpret_cast<const f4*>(base + (size_t)(az ^ 16u));
    d.ch = *reinterpret_cast<const int4*>(base + (size_t)t + 96);
}
TR_DEV void box4_test(const RayPre& r, const Node4Data& d, float tmin, float tmax, Hit4& h) {
    int c0 = d.ch.x, c1 = d.ch.y, c2 = d.ch.z, c3 = d.ch.w;
    const float nx[4] = {d.nxv.x, d.nxv.y, d.nxv.z, d.nxv.w}, ny[4] = {d.nyv.x, d.nyv.y, d.nyv.z, d.nyv.w}, nz[4] = {d.nzv.x, d.nzv.y, d.nzv.z, d.nzv.w};
    const float fx[4] = {d.fxv.x, d.fxv.y, d.fxv.z, d.fxv.w}, fy[4] = {d.fyv.x, d.fyv.y, d.fyv.z, d.fyv.w}, fz[4] = {d.fzv.x, d.fzv.y, d.fzv.z, d.fzv.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // the three slabs in the ray's axis order: max / min over them do not depend on the order
        const float tx0 = (nx[k] - r.op.x) * r.ip.x, tx1 = (fx[k] - r.op.x) * r.ip.x;
        const float ty0 = (ny[k] - r.op.y) * r.ip.y, ty1 = (fy[k] - r.op.y) * r.ip.y;
        const float tz0 = (nz[k] - r.op.z) * r.ip.z, tz1 = (fz[k] - r.op.z) * r.ip.z;
        const float t0 = fmaxf(fmaxf(tx0, ty0), fmaxf(tz0, tmin));
        const float t1 = fminf(fminf(fminf(tx1, ty1), tz1), tmax) * TR_SLAB_PAD;
        h.t[k] = t0 <= t1 ? t0 : __builtin_huge_valf();
    }
    // keeps the load of the child ids next to the plane loads: left alone, the compiler sinks it into the "some child is hit"
    // branch, one more dependent round trip per node
    asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
    h.c[0] = c0; h.c[1] = c1; h.c[2] = c2; h.c[3] = c3;
}
TR_DEV void box4_intersect(const RayPre& r, const Bvh4Node* nodes, int node, float tmin, float tmax, Hit4& h TL(, TlPhase* tlp = nullptr)) {
    Node4Data d;
    box4_load(r, nodes, node, d);
    TL(if (tlp) tlp->loads_issued();)
    box4_test(r, d, tmin, tmax, h);
}

// What the any-hit loop does with the four slab tests of a node: the first hit child in slot order is where the ray goes next, the other
// hit children go onto the stack in slot order (unordered descent: an occluder anywhere ends the ray).  Returns false without a hit.
TR_DEV bool shadow_descend(const Hit4& h, LaneStack& stk, int* spill, int& node) {
    const bool h0 = h.t[0] < __builtin_huge_valf(), h1 = h.t[1] < __builtin_huge_valf(), h2 = h.t[2] < __builtin_huge_valf(), h3 = h.t[3] < __builtin_huge_valf();
    const int n = (int)h0 + (int)h1 + (int)h2 + (int)h3;
    if (n == 0) return false;
    // registers, not elements of an array: a select between array elements is turned into a load at a selected address, which puts the array into scratch
    int c0 = h.c[0], c1 = h.c[1], c2 = h.c[2], c3 = h.c[3];
    asm volatile("" : "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
    const int first = h0 ? c0 : (h1 ? c1 : (h2 ? c2 : c3));
    // the hit children behind the first, packed to the front: a = the second hit, b = the third; `last` = the last hit, which becomes the
    // top of the stack (two hits: a; three: b; four: c3)
    const int a = (h0 && h1) ? c1 : ((h2 && (h0 != h1)) ? c2 : c3);
    const int b = (h0 && h1 && h2) ? c2 : c3;
    const int last = h3 ? c3 : (h2 ? c2 : c1);
    stk.push_packed(spill, n - 1, a, b, last);
    node = first;
    return true;
}

#define TR_CE4(a, b) { const bool sw = h.t[b] < h.t[a]; const float ta = h.t[a], tb = h.t[b]; const int ca = h.c[a], cb = h.c[b]; \
                       h.t[a] = sw ? tb : ta; h.t[b] = sw ? ta : tb; h.c[a] = sw ? cb : ca; h.c[b] = sw ? ca : cb; }

// =====================================================================================================================
// Sphere lights (rt_common_point_light.rint:11-17 / .rchit:10-15, shader/rt_common.glsl:36-51), after the triangles: every point / spot
// light with radius != 0 in a loop, or - LightTreeHeader::use_tree - a walk of the light tree.  Both give the loop's
// result bit for bit: of the lights whose fp32 root hh satisfies hh > 0, hh > tmin and hh < best_t (the closest triangle, or tmax), the
// smallest hh wins, the lowest index on equal hh; a triangle at the same t beats every light.
//
// The root as the reference computes it, in its operation order (no contraction: -ffp-contract=off).  NaN when the sphere is missed is
// not needed: disc < 0 returns -1, which no test accepts.
TR_DEV float sphere_light_root(f3 org, f3 dir, f3 pos, float radius) {
    f3 oc = org - pos;
    float a = dot(dir, dir);
    float b = 2.0f * dot(oc, dir);
    float c = dot(oc, oc) - radius * radius;
    float disc = b * b - 4.0f * a * c;
    if (disc < 0) return -1.0f;
    return (-b - sqrtf(disc)) / (2.0f * a);
}

// Leaf boxes of the light tree are pos +- (r + TR_LIGHT_KAPPA (|pos|inf + r)), and a ray widens every box it tests by TR_LIGHT_KAPPA |org|inf
// more.  Why that is enough: hh is not the geometric sphere's root.  With v = oc as computed (v = org - pos', |pos' - pos| <= eps |org - pos|
// per component, eps = 2^-24), a = |d|^2 (1 + 3 eps), b = 2 (v.d + e_b), |e_b| <= 3 eps |v||d|, c = |v|^2 - r^2 + e_c, |e_c| <= 4 eps (|v|^2 + r^2),
// the computed disc is the exact 4 |d|^2 (r^2 - dist^2) (dist: pos' to the ray's line) plus an error E with |E| <= 16 eps 4 |d|^2 (|v|^2 + r^2)
// (b^2 and 4ac are both up to 4 |d|^2 (|v|^2 + r^2) and each carries a few eps of it; far from the light they nearly cancel, which is
// why a ray that misses the sphere can still report a root).  The exact root of the quadratic with that disc lies on a sphere about pos' of
// radius sqrt(r^2 + E / (4 |d|^2)) <= r + 4 sqrt(eps) (|v| + r); rounding b, the square root, the subtraction and the division moves the
// point org + hh d along the ray by at most ~10 eps (|v| + r) more.  So |org + hh d - pos|_2 <= r + (4 sqrt(eps) + 11 eps)(|v|_2 + r), and
// with |v|_2 <= sqrt(3) (1 + eps) (|org|inf + |pos|inf) every coordinate of the point is within r + 1.692e-3 (|org|inf + |pos|inf + r) of
// pos.  TR_LIGHT_KAPPA (common.h) = 2^-9 = 1.953e-3 leaves 15 % for the rounding of the stored boxes (outwards on the host) and of the widened origins here.
// A box that contains the exact point is entered no later than hh (1 + 3 eps) and left no earlier than hh (1 - 3 eps); TR_SLAB_PAD covers
// both, so every light whose hh the loop would accept is reached (tests/test_sphere_light_accel.py checks it against the oracle).
// The bound assumes |d|^2 and the products stay in fp32's normal range (ray directions of a frame are unit vectors).
#define TR_LIGHT_STACK TR_LDS_STACK     // the walk keeps its stack in the lane's LDS column, free once the triangles are done

// Candidate light i with root hh against the best so far: selects, not a branch.
TR_DEV void consider_light(float hh, int i, float tmin, float& best_t, int& best_light) {
    const bool take = hh > 0 && hh > tmin && (hh < best_t || (hh == best_t && best_light >= 0 && i < best_light));
    best_t = take ? hh : best_t;
    best_light = take ? i : best_light;
}

template <bool COUNT>
TR_DEV void sphere_light_loop(const SceneView& sv, f3 org, f3 dir, float tmin, float& best_t, int& best_light, TraceStats& st) {
    for (uint i = 0; i < sv.point_light_count; ++i) {
        const PointLight& pl = sv.point_lights[i];
        float radius = pl.radius;
        if (radius == 0.0f) continue;
        if (COUNT) st.ltests++;
        consider_light(sphere_light_root(org, dir, pl.pos, radius), (int)i, tmin, best_t, best_light);
    }
}

// The walk of the tree.  Kept lean - one child box at a time, no sorting network, a loop the compiler does not unroll, its ray derived from
// org / dir rather than the traversal's RayPre - so that it needs few registers next to what the kernel keeps live (a walk with the
// triangle loop's four-box test and sort added spills to the closest-hit kernels).  Lights are rarely hit, so the walk has little to gain
// from visiting near children first.  `best_t` is the triangle result; returns the winning light (-1: none) and its hh in `t`.  A full
// stack reports overflow = 1 and the caller runs the loop.
struct LightWalk { float t; int light; uint tests, nodes, overflow; };
template <bool COUNT>
TR_DEV LightWalk light_tree_walk(const PointLight* lights, const Bvh4Node* nodes, f3 org, f3 dir, float tmin, float best_t, int* lds_stack) {
    int best_light = -1;
    uint tests = 0, visits = 0;
    bool overflow = false;
    // every box widened by w: near planes move towards the ray, far planes away from it (the sign of the direction picks which is which).
    // The ray's own RayPre is not kept alive for this: its values are org / dir again, in another order.
    const float w = TR_LIGHT_KAPPA * fmaxf(fmaxf(fabsf(org.x), fabsf(org.y)), fabsf(org.z));
    const f3 ip = F3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
    const uint nk = ((__float_as_uint(ip.x) >> 31) << 4) | ((32u | ((__float_as_uint(ip.y) >> 31) << 4)) << 8) | ((64u | ((__float_as_uint(ip.z) >> 31) << 4)) << 16);
    const char* base = reinterpret_cast<const char*>(nodes);
    int sp = 0, node = 0;
    while (true) {
        if (node >= 0) {
            if (COUNT) visits++;
            const uint t = (uint)node << 7;
#pragma unroll 1
            for (uint k = 0; k < 4; ++k) {
                const uint ax = t + (nk & 0xFFu) + 4u * k, ay = t + ((nk >> 8) & 0xFFu) + 4u * k, az = t + (nk >> 16) + 4u * k;
                const float nx = *reinterpret_cast<const float*>(base + ax), fx = *reinterpret_cast<const float*>(base + (ax ^ 16u));
                const float ny = *reinterpret_cast<const float*>(base + ay), fy = *reinterpret_cast<const float*>(base + (ay ^ 16u));
                const float nz = *reinterpret_cast<const float*>(base + az), fz = *reinterpret_cast<const float*>(base + (az ^ 16u));
                const int c = *reinterpret_cast<const int*>(base + t + 96u + 4u * k);
                const float wx = copysignf(w, ip.x), wy = copysignf(w, ip.y), wz = copysignf(w, ip.z);
                const float t0 = fmaxf(fmaxf((nx - (org.x + wx)) * ip.x, (ny - (org.y + wy)) * ip.y), fmaxf((nz - (org.z + wz)) * ip.z, tmin));
                const float t1 = fminf(fminf(fminf((fx - (org.x - wx)) * ip.x, (fy - (org.y - wy)) * ip.y), (fz - (org.z - wz)) * ip.z), best_t) * TR_SLAB_PAD;
                if (t0 <= t1) {     // empty slots hold an inverted box and never pass
                    if (sp < TR_LIGHT_STACK) lds_stack[sp * TR_BLOCK] = c;
                    overflow = overflow || sp >= TR_LIGHT_STACK;
                    sp = sp < TR_LIGHT_STACK ? sp + 1 : sp;
                }
            }
        } else {
            const int i = ~node;
            const PointLight& pl = lights[i];
            if (COUNT) tests++;
            if (pl.radius != 0.0f) consider_light(sphere_light_root(org, dir, pl.pos, pl.radius), i, tmin, best_t, best_light);
        }
        if (sp == 0) break;
        --sp;
        node = lds_stack[sp * TR_BLOCK];
    }
    return {best_t, best_light, tests, visits, overflow ? 1u : 0u};
}

// The sphere lights of a closest-hit ray whose triangles are done: `best_t` is the closest triangle's t, or tmax without one.  Returns the
// winning light (-1: none, the triangle result stands) and its hh, which is the hit's t and u.  The kernels call this after the triangle
// traversal has returned and its hit is stored, with the ray read again from memory: nothing of the walk or of the light result is live
// across the triangle loops (run inside them, the walk cost those loops spills).  The caller checks that the ray is finite, as the
// traversal does.
struct LightHit { float t; int light; };
template <bool COUNT>
TR_DEV LightHit trace_sphere_lights(const SceneView& sv, f3 org, f3 dir, float tmin, float best_t, int* lds_stack, TraceStats& st) {
    int best_light = -1;
    if (sv.point_light_count == 0) return {best_t, best_light};
    bool fallback = light_tree_header(sv)->use_tree == 0u;
    if (!fallback) {
        const LightWalk lw = light_tree_walk<COUNT>(sv.point_lights, light_tree_nodes(sv), org, dir, tmin, best_t, lds_stack);
        best_t = lw.t; best_light = lw.light;
        if (COUNT) { st.ltests += lw.tests; st.lnodes += lw.nodes; st.lfallbacks += lw.overflow; }
        fallback = lw.overflow != 0u;
    }
    // no tree, or a walk that ran out of stack: the loop over every light (same rule, so a partial walk before it changes nothing)
    if (fallback) sphere_light_loop<COUNT>(sv, org, dir, tmin, best_t, best_light, st);
    return {best_t, best_light};
}

// =====================================================================================================================
// Two-level structures: what the per-lane loops below do with TWO_LEVEL = true.  A TLAS leaf is a node-phase step
// that moves the ray into the instance's object space and descends into its BLAS, with a sentinel on the stack below the BLAS entries
// that brings the world ray back when it is popped.  The object-space ray is M^-1 (o, 1) and M^-1 (d, 0), not renormalised: a point at
// distance t along it is the image of the world point at t, so t, the culling bound best_t and the candidate order (t, instance,
// primitive) keep their meaning across instances.
#define TR_BLAS_SENTINEL 0x7FFFFFFF   // the reference of an empty child slot, which no node phase ever pushes

struct InstanceFrame { uint inst_word, alpha_base; };

// The ray of TLAS leaf `leaf` in its BLAS: the world ray for an identity leaf, else M^-1 applied in a fixed order.
TR_DEV int enter_instance(const SceneView& sv, int leaf, f3 org, f3 dir, const RayPre& rw, RayPre& r, InstanceFrame& fr) {
    const TlasLeaf* L = tlas_leaves(sv) + leaf;
    const f4* q = reinterpret_cast<const f4*>(L);
    const f4 a = q[0], b = q[1], c = q[2];
    const int4 w = *reinterpret_cast<const int4*>(q + 3);
    fr.inst_word = (uint)w.y; fr.alpha_base = (uint)w.z;
    if ((uint)w.w & TR_TLAS_IDENTITY) r = rw;
    else {
        const f3 o = F3(a.x * org.x + a.y * org.y + a.z * org.z + a.w, b.x * org.x + b.y * org.y + b.z * org.z + b.w,
                        c.x * org.x + c.y * org.y + c.z * org.z + c.w);
        const f3 d = F3(a.x * dir.x + a.y * dir.y + a.z * dir.z, b.x * dir.x + b.y * dir.y + b.z * dir.z, c.x * dir.x + c.y * dir.y + c.z * dir.z);
        r = make_ray(o, d);
    }
    return w.x;
}
// the words of a BLAS record as the instance the ray is in sees them
TR_DEV void instance_words(const InstanceFrame& fr, TriHit& tr) {
    if (fr.inst_word == TR_INST_FROM_RECORD) return;
    tr.inst_flags = fr.inst_word;
    tr.alpha = 0x80000000u | (fr.alpha_base + tr.prim);
}

// Closest hit over triangles, one ray per lane (sphere lights: trace_sphere_lights, called after it).  ALPHA_MODE 0: stochastic alpha keyed by `seed`
// (shader/rt_common.rahit:15-24); 1: fixed cutoff 1e-4 (shader/rt_feature.rahit:17).  One loop for both structure kinds: a one-level
// ray starts inside "its BLAS" (the whole tree) and never leaves it, a two-level ray starts in the TLAS.
template <int ALPHA_MODE, bool COUNT, bool TWO_LEVEL = false>
TR_DEV void trace_closest4(const SceneView& sv, f3 org, f3 dir, float tmin, float tmax, uint seed,
                           int* lds_stack, HitRecord& hit, TraceStats& st, int& overflow) {
    hit.instance_id = -1; hit.primitive_id = -1; hit.u = 0; hit.v = 0; hit.t = -1.0f;
    float best_t = tmax;
    bool found = false;
    uint best_inst = 0xFFFFFFFFu, best_prim = 0xFFFFFFFFu;
    const RayPre rw = make_ray(org, dir);
    RayPre r = rw;
    const bool finite_ray = ray_is_finite(org, dir);
    if (sv.tri_count > 0 && finite_ray) {
        LaneStack stk;
        int spill[TR_SPILL_STACK];
        stk.init(lds_stack);
        int node = TWO_LEVEL ? 0 : (sv.node_count > 0 ? 0 : -1);   // one level, single-triangle scene: leaf ~0 == -1
        bool in_blas = !TWO_LEVEL;
        InstanceFrame fr = {0u, 0u};
        while (true) {
            const bool at_tri = node < 0 && in_blas;
#if TR_VOTE > 0
            const int n_leaf = __popcll(__ballot(at_tri)), n_all = __popcll(__ballot(true));
            const bool leaf_phase = n_leaf >= TR_VOTE || n_leaf == n_all;
            if (at_tri != leaf_phase) continue;
#endif
            if (COUNT && !TWO_LEVEL) {
                const unsigned long long m = __ballot(true), mn = __ballot(node >= 0);
                if ((int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) {
                    if (mn) { st.ph_node++; if (__popcll(m) <= 16) { st.ph_node16++; st.lv_node16 += (uint)__popcll(mn); } if (__popcll(m) <= 8) st.ph_node8++; }
                    else st.ph_tri++;
                }
            }
            if (!at_tri) {
                if (node >= 0) {
                    Hit4 h;
                    box4_intersect(r, sv.nodes4, node, tmin, best_t, h);
                    if (COUNT) st.nodes++;
                    TR_CE4(0, 1) TR_CE4(2, 3) TR_CE4(0, 2) TR_CE4(1, 3) TR_CE4(1, 2)
                    if (h.t[0] < __builtin_huge_valf()) {
                        // sorted: the hit children come first, so the number of further hits says which of c[1..3] go onto the stack
                        const int m = (int)(h.t[1] < __builtin_huge_valf()) + (int)(h.t[2] < __builtin_huge_valf()) + (int)(h.t[3] < __builtin_huge_valf());
                        stk.push_sorted(spill, m, h.c[1], h.c[2], h.c[3]);
                        if (COUNT) st.maxsp = max(st.maxsp, (uint)stk.sp);
                        node = h.c[0];
                        continue;
                    }
                } else if constexpr (TWO_LEVEL) {    // TLAS leaf: into the instance
                    stk.push(spill, TR_BLAS_SENTINEL);
                    if (COUNT) st.maxsp = max(st.maxsp, (uint)stk.sp);
                    node = enter_instance(sv, ~node, org, dir, rw, r, fr);
                    in_blas = true;
                    continue;
                }
            } else {
                TriHit tr;
                if (COUNT) st.tris++;
                if (tri_intersect(r, sv.tris, (uint)~node, tmin, __builtin_huge_valf(), tr)) {
                    if constexpr (TWO_LEVEL) instance_words(fr, tr);
                    const float t = tr.t, bu = tr.bu, bv = tr.bv;
                    const uint inst = tr.inst_flags & 0x7FFFFFFFu;
                    const bool closer = t < best_t ||
                        (t == best_t && found && (inst < best_inst || (inst == best_inst && tr.prim < best_prim)));
                    if (closer && t < tmax) {
                        bool accept = true;
                        if (tr.inst_flags & 0x80000000u) {
                            if (COUNT) st.alpha++;
                            float a = candidate_alpha(sv, tr.alpha, bu, bv);
                            float cutoff = ALPHA_MODE == 0 ? alpha_cutoff_hash(seed, (int)inst, (int)tr.prim) : 0.0001f;
                            accept = !(a <= cutoff);
                        }
                        if (accept) {
                            best_t = t; found = true; best_inst = inst; best_prim = tr.prim;
                            hit.instance_id = (int)inst; hit.primitive_id = (int)tr.prim; hit.u = bu; hit.v = bv;
                        }
                    }
                }
            }
            if (stk.sp == 0) break;
            node = stk.pop(spill);
            if constexpr (TWO_LEVEL) {
                if (node == TR_BLAS_SENTINEL) {     // the BLAS is done: back to the world ray (below a sentinel lies a TLAS entry or nothing)
                    r = rw; in_blas = false;
                    if (stk.sp == 0) break;
                    node = stk.pop(spill);
                }
            }
        }
        overflow += stk.overflow ? 1 : 0;
    }
    hit.t = found ? best_t : -1.0f;
}

// shadow_ray (shader/path_tracer.glsl:35-52) + rt_common_shadow.rahit/.rchit: product of (1 - alpha)
// over non-opaque hits, 0 on the first opaque hit; lights are excluded (mask 0xFD).
template <bool COUNT, bool TWO_LEVEL = false>
TR_DEV float trace_shadow4(const SceneView& sv, f3 org, f3 dir, float tmin, float tmax, int* lds_stack, TraceStats& st, int& overflow) {
    float visibility = 1.0f;
    if (sv.tri_count == 0 || !ray_is_finite(org, dir)) return visibility;
    const RayPre rw = make_ray(org, dir);
    RayPre r = rw;
    LaneStack stk;
    int spill[TR_SPILL_STACK];
    stk.init(lds_stack);
    int node = TWO_LEVEL ? 0 : (sv.node_count > 0 ? 0 : -1);   // one level, single-triangle scene: leaf ~0 == -1
    bool in_blas = !TWO_LEVEL;
    InstanceFrame fr = {0u, 0u};
    while (true) {
        if (node >= 0) {
            Hit4 h;
            box4_intersect(r, sv.nodes4, node, tmin, tmax, h);
            if (COUNT) st.nodes++;
            if (shadow_descend(h, stk, spill, node)) continue;
        } else if (!in_blas) {      // TLAS leaf: into the instance (a one-level ray is never outside)
            if constexpr (TWO_LEVEL) {
                stk.push(spill, TR_BLAS_SENTINEL);
                node = enter_instance(sv, ~node, org, dir, rw, r, fr);
                in_blas = true;
                continue;
            }
        } else {
            TriHit tr;
            if (COUNT) st.tris++;
            if (tri_intersect(r, sv.tris, (uint)~node, tmin, tmax, tr)) {
                if constexpr (TWO_LEVEL) instance_words(fr, tr);
                if (!(tr.inst_flags & 0x80000000u)) { visibility = 0.0f; break; }
                if (COUNT) st.alpha++;
                float alpha = candidate_alpha(sv, tr.alpha, tr.bu, tr.bv);
                visibility *= 1.0f - alpha;
                if (visibility == 0.0f) break;
            }
        }
        if (stk.sp == 0) break;
        node = stk.pop(spill);
        if constexpr (TWO_LEVEL) {
            if (node == TR_BLAS_SENTINEL) {
                r = rw; in_blas = false;
                if (stk.sp == 0) break;
                node = stk.pop(spill);
            }
        }
    }
    overflow += stk.overflow ? 1 : 0;
    return visibility;
}

// LDS words per block for the per-lane stacks: TR_LDS_STACK rows and, in front of them, the row a store to "row -1" lands in (LaneStack).
// Kernels declare `__shared__ int s_stack_rows[TR_STACK_WORDS]` and hand out `s_stack_rows + TR_STACK_ROW0`.
#define TR_STACK_ROW0 TR_BLOCK
#define TR_STACK_WORDS ((TR_LDS_STACK + 1) * TR_BLOCK)

}  // namespace tr
