// On-device acceleration-structure build: the software replacement for the driver's BLAS/TLAS build
// (reference call sites src/acceleration_structure.cc:198,266,421; recorded by src/scene_stage.cc:1620-1662).
//   world triangles (model * vec4(pos, 1), GLSL order) + centroid bounds -> 63-bit Morton keys -> radix sort (rocPRIM)
//   -> PLOC clustering over the Morton order (or Karras 2012 LBVH + atomic refit, TRHIP_BUILDER=lbvh)
//   -> depth-first relabelling -> in-place collapse to 4-wide fp32 nodes (128 B) + 48-byte triangle records.
// trhip_scene_refit_accel keeps the tree and recomputes its boxes level by level.  Also here: extract_tri_lights
// (shader/extract_tri_lights.comp:17-54) and the pre-transformed vertex copy (shader/pre_transform.comp:26-42).
#include <algorithm>
#include <cctype>
#include <chrono>
#include <cmath>
#include <map>
#include <tuple>
#include <vector>
#include "build.h"

#include <rocprim/rocprim.hpp>

namespace tr {

namespace {

constexpr int BT = 256;

// order-preserving float <-> uint map for atomicMin/Max on bounds
TR_DEV uint float_flip(float f) { uint u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
TR_HD float float_unflip(uint u) {
    uint v = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float f;
#if defined(__HIP_DEVICE_COMPILE__)
    f = __uint_as_float(v);
#else
    memcpy(&f, &v, 4);
#endif
    return f;
}

// instance/primitive of a global triangle id via binary search over the per-instance prefix sums
TR_DEV void locate_triangle(const uint* tri_prefix, uint instance_count, uint gid, uint& inst, uint& prim) {
    uint lo = 0, hi = instance_count;   // prefix has instance_count + 1 entries
    while (hi - lo > 1) {
        uint mid = (lo + hi) >> 1;
        if (tri_prefix[mid] <= gid) lo = mid; else hi = mid;
    }
    inst = lo;
    prim = gid - tri_prefix[lo];
}

// TriRecord::alpha of a triangle of a non-opaque instance, and its AlphaTri record (common.h).  The material can change between a build
// and a refit (trhip_scene_update_instances replaces the whole instance record), so both write it.
TR_DEV uint alpha_word(const Material& mat, uint record, AlphaTri* alpha_tris, f2 uv0, f2 uv1, f2 uv2) {
    AlphaTri a;
    a.uv0 = uv0; a.uv1 = uv1; a.uv2 = uv2; a.factor = mat.albedo_factor.w; a.tex = mat.albedo_tex_id;
    alpha_tris[record] = a;
    const uint bits = __float_as_uint(a.factor);
    return (a.tex < 0 && !(bits & 0x80000000u)) ? bits : (0x80000000u | record);
}

// world-space triangle = (model * vec4(pos, 1)).xyz in the GLSL evaluation order; also accumulates the
// centroid bounds used to quantise Morton codes.
__global__ __launch_bounds__(BT) void k_pretransform(SceneView sv, const uint* tri_prefix, const uint8_t* non_opaque, const uint* alpha_base, AlphaTri* alpha_tris,
                                                     TriRecord* tris_unsorted, uint* cbounds /*6 flipped uints of the centroid bounds; [16..21] the same for the triangles' bounds*/) {
    float cmin[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float cmax[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    float smin[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float smax[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    // a bounded grid walks the triangles: the twelve bounds end in twelve atomics per block on two cache lines, and 16 000 waves of
    // them (one set per wave of a grid of one thread per triangle) took a millisecond of a 4 ms rebuild - the atomics of a line are
    // served one after the other ("Atomics")
    for (uint gid = blockIdx.x * BT + threadIdx.x; gid < sv.tri_count; gid += gridDim.x * BT) {
        uint inst, prim;
        locate_triangle(tri_prefix, sv.instance_count, gid, inst, prim);
        const MeshSpan sp = sv.spans[inst];
        const uint* ix = sv.indices + sp.index_offset + 3u * prim;
        const Vertex* vb = sv.vertices + sp.vertex_offset;
        const m4 model = sv.instances[inst].model;
        f3 p0 = transform_point(model, vb[ix[0]].pos);
        f3 p1 = transform_point(model, vb[ix[1]].pos);
        f3 p2 = transform_point(model, vb[ix[2]].pos);
        TriRecord t;
        t.v0[0] = p0.x; t.v0[1] = p0.y; t.v0[2] = p0.z;
        t.v1[0] = p1.x; t.v1[1] = p1.y; t.v1[2] = p1.z;
        t.v2[0] = p2.x; t.v2[1] = p2.y; t.v2[2] = p2.z;
        t.inst_flags = inst | (non_opaque[inst] ? 0x80000000u : 0u);
        t.prim = prim;
        t.alpha = non_opaque[inst] ? alpha_word(sv.instances[inst].mat, alpha_base[inst] + prim, alpha_tris, vb[ix[0]].uv, vb[ix[1]].uv, vb[ix[2]].uv) : 0u;
        tris_unsorted[gid] = t;
        f3 lo = min3(min3(p0, p1), p2), hi = max3(max3(p0, p1), p2);
        f3 c = (lo + hi) * 0.5f;
        const float cc[3] = {c.x, c.y, c.z}, ll[3] = {lo.x, lo.y, lo.z}, hh[3] = {hi.x, hi.y, hi.z};
        for (int k = 0; k < 3; ++k) { cmin[k] = fminf(cmin[k], cc[k]); cmax[k] = fmaxf(cmax[k], cc[k]); smin[k] = fminf(smin[k], ll[k]); smax[k] = fmaxf(smax[k], hh[k]); }
    }
    // wave reduce, block reduce through LDS, then one set of atomics per block
    __shared__ float s_red[BT / 64][12];
    for (int k = 0; k < 3; ++k) {
        float mn = cmin[k], mx = cmax[k], sn = smin[k], sx = smax[k];
        for (int off = 32; off > 0; off >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, off));
            mx = fmaxf(mx, __shfl_xor(mx, off));
            sn = fminf(sn, __shfl_xor(sn, off));
            sx = fmaxf(sx, __shfl_xor(sx, off));
        }
        if ((threadIdx.x & 63) == 0) { float* w = s_red[threadIdx.x >> 6]; w[k] = mn; w[3 + k] = mx; w[6 + k] = sn; w[9 + k] = sx; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = (int)threadIdx.x;
        float mn = s_red[0][k], mx = s_red[0][3 + k], sn = s_red[0][6 + k], sx = s_red[0][9 + k];
        for (int w = 1; w < BT / 64; ++w) { mn = fminf(mn, s_red[w][k]); mx = fmaxf(mx, s_red[w][3 + k]); sn = fminf(sn, s_red[w][6 + k]); sx = fmaxf(sx, s_red[w][9 + k]); }
        if (mn <= mx) {
            atomicMin(&cbounds[k], float_flip(mn));
            atomicMax(&cbounds[3 + k], float_flip(mx));
            atomicMin(&cbounds[16 + k], float_flip(sn));     // bounds of the triangles themselves: the grid of the pre-split
            atomicMax(&cbounds[19 + k], float_flip(sx));
        }
    }
}

TR_DEV unsigned long long expand21(uint v) {   // spread 21 bits to every third bit
    unsigned long long x = v & 0x1FFFFFull;
    x = (x | x << 32) & 0x1F00000000FFFFull;
    x = (x | x << 16) & 0x1F0000FF0000FFull;
    x = (x | x << 8) & 0x100F00F00F00F00Full;
    x = (x | x << 4) & 0x10C30C30C30C30C3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

__global__ __launch_bounds__(BT) void k_morton(uint n, const TriRecord* tris, const uint* cbounds, unsigned long long* keys, uint* vals) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    float lo[3], inv[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = float_unflip(cbounds[k]);
        float ext = float_unflip(cbounds[3 + k]) - lo[k];
        inv[k] = ext > 0 ? 2097151.0f / ext : 0.0f;
    }
    const TriRecord t = tris[i];
    float c[3];
    for (int k = 0; k < 3; ++k) {
        float mn = fminf(fminf(t.v0[k], t.v1[k]), t.v2[k]), mx = fmaxf(fmaxf(t.v0[k], t.v1[k]), t.v2[k]);
        c[k] = (mn + mx) * 0.5f;
    }
    uint q[3];
    for (int k = 0; k < 3; ++k) {
        float f = (c[k] - lo[k]) * inv[k];
        q[k] = (uint)fminf(fmaxf(f, 0.0f), 2097151.0f);
    }
    keys[i] = (expand21(q[0]) << 2) | (expand21(q[1]) << 1) | expand21(q[2]);
    vals[i] = i;
}

// Karras 2012: common-prefix length between sorted keys i and j, ties broken by index
TR_DEV int delta(const unsigned long long* keys, int n, int i, int j) {
    if (j < 0 || j >= n) return -1;
    unsigned long long a = keys[i], b = keys[j];
    if (a == b) return 64 + __clz((uint)i ^ (uint)j);
    return __clzll((long long)(a ^ b));
}

// one thread per internal node i in [0, n-1): children + parent links.
// refs: >= 0 internal node, < 0 leaf ~leaf_index (leaf_index = position in sorted order)
__global__ __launch_bounds__(BT) void k_hierarchy(int n, const unsigned long long* keys, int2* children, uint* subtree_size, int* parent_internal, int* parent_leaf) {
    int i = blockIdx.x * BT + threadIdx.x;
    if (i >= n - 1) return;
    int d = (delta(keys, n, i, i + 1) - delta(keys, n, i, i - 1)) >= 0 ? 1 : -1;
    int dmin = delta(keys, n, i, i - d);
    int lmax = 2;
    while (delta(keys, n, i, i + lmax * d) > dmin) lmax <<= 1;
    int l = 0;
    for (int t = lmax >> 1; t >= 1; t >>= 1)
        if (delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
    int j = i + l * d;
    int dnode = delta(keys, n, i, j);
    int s = 0;
    int t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    int gamma = i + s * d + min(d, 0);
    int left = (min(i, j) == gamma) ? ~gamma : gamma;
    int right = (max(i, j) == gamma + 1) ? ~(gamma + 1) : (gamma + 1);
    children[i] = make_int2(left, right);
    subtree_size[i] = (uint)(max(i, j) - min(i, j) + 1);   // leaves covered by this node
    if (left >= 0) parent_internal[left] = i; else parent_leaf[~left] = i;
    if (right >= 0) parent_internal[right] = i; else parent_leaf[~right] = i;
    if (i == 0) parent_internal[0] = -1;
}

// gather triangles into Morton order and emit leaf boxes
__global__ __launch_bounds__(BT) void k_gather_leaves(uint n, const TriRecord* unsorted, const uint* sorted_vals, TriRecord* sorted, float* leaf_box /*6 per leaf*/) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    const TriRecord t = unsorted[sorted_vals[i]];
    sorted[i] = t;
    for (int k = 0; k < 3; ++k) {
        leaf_box[6 * i + k] = fminf(fminf(t.v0[k], t.v1[k]), t.v2[k]);
        leaf_box[6 * i + 3 + k] = fmaxf(fmaxf(t.v0[k], t.v1[k]), t.v2[k]);
    }
}

// bottom-up refit: the second thread to reach a node owns it.  Agent-scope release/acquire around the
// arrival counter makes the first child's box (written by another CU, possibly another XCD) visible.
__global__ __launch_bounds__(BT) void k_refit(int n, const int2* children, const int* parent_internal, const int* parent_leaf,
                                              const float* leaf_box, float* node_box /*6 per internal*/, uint* arrive, BvhNode* nodes) {
    int leaf = blockIdx.x * BT + threadIdx.x;
    if (leaf >= n) return;
    int node = parent_leaf[leaf];
    while (node >= 0) {
        __threadfence();   // release: our child's box is published before we announce arrival
        uint prev = __hip_atomic_fetch_add(&arrive[node], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == 0) return;            // sibling subtree not finished: the other thread continues
        __threadfence();   // acquire
        const int2 ch = children[node];
        BvhNode out;
        float lo[3], hi[3];
        {
            const float* b0 = ch.x >= 0 ? node_box + 6 * (size_t)ch.x : leaf_box + 6 * (size_t)(~ch.x);
            const float* b1 = ch.y >= 0 ? node_box + 6 * (size_t)ch.y : leaf_box + 6 * (size_t)(~ch.y);
            for (int k = 0; k < 3; ++k) {
                float l0 = __hip_atomic_load(&b0[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                float h0 = __hip_atomic_load(&b0[3 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                float l1 = __hip_atomic_load(&b1[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                float h1 = __hip_atomic_load(&b1[3 + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                out.lo0[k] = l0; out.hi0[k] = h0; out.lo1[k] = l1; out.hi1[k] = h1;
                lo[k] = fminf(l0, l1); hi[k] = fmaxf(h0, h1);
            }
        }
        out.child0 = ch.x; out.child1 = ch.y; out.pad0 = 0; out.pad1 = 0;
        nodes[node] = out;
        for (int k = 0; k < 3; ++k) {
            __hip_atomic_store(&node_box[6 * (size_t)node + k], lo[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&node_box[6 * (size_t)node + 3 + k], hi[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        node = parent_internal[node];
    }
}


// ---------------------------------------------------------------------------------------------------------------
// PLOC (parallel locally-ordered clustering, Meister & Bittner 2018) on the Morton-sorted leaves: every cluster
// looks for the neighbour within +-PLOC_RADIUS positions whose merged box has the smallest area; mutual nearest
// neighbours merge; the cluster array is compacted and the round repeats until one cluster is left.  Gives
// near-SAH trees while staying a radix-sort-based on-device build.  Internal node ids are handed out from the top
// so that the last merge (the root) is node 0.
#define PLOC_RADIUS 16

TR_DEV float merged_area(const float* a, const float* b) {
    float dx = fmaxf(a[3], b[3]) - fminf(a[0], b[0]);
    float dy = fmaxf(a[4], b[4]) - fminf(a[1], b[1]);
    float dz = fmaxf(a[5], b[5]) - fminf(a[2], b[2]);
    return dx * dy + dy * dz + dz * dx;
}

// The live cluster count of a round sits in device memory (c_ptr): the host only learns it every few rounds and sizes
// the grids by its last known value, so a round costs launches but no host round trip.
__global__ __launch_bounds__(BT) void k_ploc_nn(const uint* c_ptr, uint radius, const float* cbox, uint* nn) {
    const uint c = *c_ptr;
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= c) return;
    float mine[6];
    for (int k = 0; k < 6; ++k) mine[k] = cbox[6 * (size_t)i + k];
    uint lo = i > radius ? i - radius : 0, hi = min(c - 1, i + radius);
    float best = __builtin_huge_valf(); uint bj = i;
    for (uint j = lo; j <= hi; ++j) {
        if (j == i) continue;
        float a = merged_area(mine, cbox + 6 * (size_t)j);
        if (a < best) { best = a; bj = j; }
    }
    nn[i] = bj;
}

__global__ __launch_bounds__(BT) void k_ploc_merge(const uint* c_ptr, uint n_leaves, const int* cref, const float* cbox, const uint* nn, uint* valid, int* out_ref,
                                                   float* out_box, uint* alloc, int2* children, float* node_box, uint* subtree_size, int* parent_internal) {
    const uint c = *c_ptr;
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= c) { if (i < gridDim.x * BT) valid[i] = 0; return; }   // keeps the scan input defined past the live range
    uint j = nn[i];
    const bool mutual = j != i && nn[j] == i;
    if (mutual && i > j) { valid[i] = 0; return; }
    int ref = cref[i];
    float box[6];
    for (int k = 0; k < 6; ++k) box[k] = cbox[6 * (size_t)i + k];
    if (mutual) {
        const int other = cref[j];
        const float* ob = cbox + 6 * (size_t)j;
        for (int k = 0; k < 3; ++k) { box[k] = fminf(box[k], ob[k]); box[3 + k] = fmaxf(box[3 + k], ob[3 + k]); }
        const uint id = (n_leaves - 2u) - atomicAdd(alloc, 1u);
        children[id] = make_int2(ref, other);
        if (ref >= 0) parent_internal[ref] = (int)id;
        if (other >= 0) parent_internal[other] = (int)id;
        for (int k = 0; k < 6; ++k) node_box[6 * (size_t)id + k] = box[k];
        subtree_size[id] = (ref < 0 ? 1u : subtree_size[ref]) + (other < 0 ? 1u : subtree_size[other]);
        ref = (int)id;
    }
    valid[i] = 1;
    out_ref[i] = ref;
    for (int k = 0; k < 6; ++k) out_box[6 * (size_t)i + k] = box[k];
}

__global__ __launch_bounds__(BT) void k_ploc_compact(const uint* c_ptr, uint* c_next, const uint* valid, const uint* pos, const int* in_ref, const float* in_box,
                                                     int* cref, float* cbox) {
    const uint c = *c_ptr;
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= c) return;
    if (i == c - 1) *c_next = pos[i] + valid[i];   // cluster count of the next round
    if (!valid[i]) return;
    uint p = pos[i];
    cref[p] = in_ref[i];
    for (int k = 0; k < 6; ++k) cbox[6 * (size_t)p + k] = in_box[6 * (size_t)i + k];
}

// The last rounds in one workgroup: once PLOC_TAIL clusters or fewer are left, a round of three grid launches and a scan is all
// launch latency (a 1 M triangle build spent about thirty of its seventy-odd rounds there, 20-30 us each).  The clusters move into LDS, one per
// thread, and the same three steps - nearest neighbour, merge of the mutual pairs, compaction - repeat between barriers until one
// cluster is left.  Same neighbour choice (ascending scan, first minimum wins) and same merge rule as the grid kernels, so the
// same tree; node ids come from the same allocator.
#define PLOC_TAIL 1024
__global__ __launch_bounds__(PLOC_TAIL) void k_ploc_tail(const uint* c_ptr, uint n_leaves, uint radius, const int* cref, const float* cbox, uint* alloc, int2* children,
                                                         float* node_box, uint* subtree_size, int* parent_internal, uint* rounds_out) {
    __shared__ float s_box[6][PLOC_TAIL];
    __shared__ int s_ref[PLOC_TAIL];
    __shared__ uint s_nn[PLOC_TAIL];
    __shared__ uint s_wave[PLOC_TAIL / 64];
    const uint i = threadIdx.x, lane = i & 63u, w = i >> 6;
    uint c = *c_ptr;
    if (i < c) {
        s_ref[i] = cref[i];
        for (int k = 0; k < 6; ++k) s_box[k][i] = cbox[6 * (size_t)i + k];
    }
    __syncthreads();
    uint rounds = 0;
    while (c > 1) {
        uint bj = i;
        float mine[6];
        if (i < c) {
            for (int k = 0; k < 6; ++k) mine[k] = s_box[k][i];
            const uint lo = i > radius ? i - radius : 0, hi = min(c - 1, i + radius);
            float best = __builtin_huge_valf();
            for (uint j = lo; j <= hi; ++j) {
                if (j == i) continue;
                const float other[6] = {s_box[0][j], s_box[1][j], s_box[2][j], s_box[3][j], s_box[4][j], s_box[5][j]};
                const float a = merged_area(mine, other);
                if (a < best) { best = a; bj = j; }
            }
        }
        s_nn[i] = bj;
        __syncthreads();
        bool keep = false;
        int ref = 0;
        if (i < c) {
            const uint j = bj;
            const bool mutual = j != i && s_nn[j] == i;
            if (!(mutual && i > j)) {
                keep = true;
                ref = s_ref[i];
                if (mutual) {
                    const int other = s_ref[j];
                    for (int k = 0; k < 3; ++k) { mine[k] = fminf(mine[k], s_box[k][j]); mine[3 + k] = fmaxf(mine[3 + k], s_box[3 + k][j]); }
                    const uint id = (n_leaves - 2u) - atomicAdd(alloc, 1u);
                    children[id] = make_int2(ref, other);
                    if (ref >= 0) parent_internal[ref] = (int)id;
                    if (other >= 0) parent_internal[other] = (int)id;
                    for (int k = 0; k < 6; ++k) node_box[6 * (size_t)id + k] = mine[k];
                    subtree_size[id] = (ref < 0 ? 1u : subtree_size[ref]) + (other < 0 ? 1u : subtree_size[other]);
                    ref = (int)id;
                }
            }
        }
        const unsigned long long kept = __ballot(keep);
        if (lane == 0) s_wave[w] = (uint)__popcll(kept);
        __syncthreads();   // every read of this round's clusters is done, and the subtree sizes written above are visible to the block
        uint before = 0, total = 0;
        for (uint k = 0; k < PLOC_TAIL / 64; ++k) { const uint v = s_wave[k]; total += v; before += k < w ? v : 0u; }
        if (keep) {
            const uint p = before + (uint)__popcll(kept & ((1ull << lane) - 1ull));
            s_ref[p] = ref;
            for (int k = 0; k < 6; ++k) s_box[k][p] = mine[k];
        }
        c = total;
        ++rounds;
        __syncthreads();
    }
    if (i == 0) *rounds_out = rounds;
}

__global__ __launch_bounds__(BT) void k_ploc_init(uint n, int* cref) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i < n) cref[i] = ~(int)i;
}

__global__ __launch_bounds__(BT) void k_identity(uint n, int* v) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i < n) v[i] = (int)i;
}

// Depth-first relabelling: a node's slot is its pre-order index among the internal nodes, so a left child sits right
// after its parent and every subtree is one contiguous run of 64-byte nodes (keeps the lower levels of one ray's walk
// within a few cache lines / one TLB page instead of scattered by merge order).
__global__ __launch_bounds__(BT) void k_dfs_order(uint n_internal, const int2* children, const uint* subtree_size, const int* parent_internal, int* new_id) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= n_internal) return;
    uint pos = 0;
    int cur = (int)i;
    for (int p = parent_internal[cur]; p >= 0; cur = p, p = parent_internal[cur]) {
        const int2 ch = children[p];
        pos += 1u;
        if (ch.y == cur && ch.x >= 0) pos += subtree_size[ch.x] - 1u;   // skip the left subtree's internal nodes
    }
    new_id[i] = (int)pos;
}

// 64-byte traversal nodes from (children, boxes)
__global__ __launch_bounds__(BT) void k_emit_nodes(uint n_internal, const int2* children, const float* node_box, const float* leaf_box, const int* new_id,
                                                   BvhNode* nodes) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= n_internal) return;
    const int2 ch = children[i];
    const float* b0 = ch.x >= 0 ? node_box + 6 * (size_t)ch.x : leaf_box + 6 * (size_t)(~ch.x);
    const float* b1 = ch.y >= 0 ? node_box + 6 * (size_t)ch.y : leaf_box + 6 * (size_t)(~ch.y);
    BvhNode out;
    for (int k = 0; k < 3; ++k) { out.lo0[k] = b0[k]; out.hi0[k] = b0[3 + k]; out.lo1[k] = b1[k]; out.hi1[k] = b1[3 + k]; }
    out.child0 = ch.x >= 0 ? new_id[ch.x] : ch.x;
    out.child1 = ch.y >= 0 ? new_id[ch.y] : ch.y;
    out.pad0 = 0; out.pad1 = 0;
    nodes[new_id[i]] = out;
}

}  // namespace
}  // namespace tr
#include "bvh_optimize.h"
namespace tr {
namespace {

// BVH2 -> BVH4, in place: every binary node keeps its (depth-first) index and adopts up to four descendants: the ones
// k_collapse_cost chose (`dec`: least sum of 4-wide node areas), or - dec = nullptr, TRHIP_COLLAPSE=greedy - found by
// repeatedly opening the adopted inner node with the largest box.  Nodes that were adopted away are never referenced
// again; they stay as dead 128-byte lines, which costs memory but neither bandwidth nor cache (a node is one line).
__global__ __launch_bounds__(BT) void k_collapse4(uint n_internal, const int2* children, const float* node_box, const float* leaf_box, const int* new_id,
                                                  const uint8_t* dec, Bvh4Node* nodes4) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= n_internal) return;
    constexpr int W = 4;
    int cand[W];
    cand[0] = children[i].x; cand[1] = children[i].y;
    int ncand = 2;
    if (dec) ncand = collapse_children(children, dec, (int)i, cand);
    while (!dec && ncand < W) {
        int best = -1; float best_area = -1.0f;
        for (int c = 0; c < ncand; ++c) {
            if (cand[c] < 0) continue;
            const float* b = node_box + 6 * (size_t)cand[c];
            float dx = b[3] - b[0], dy = b[4] - b[1], dz = b[5] - b[2];
            float area = dx * dy + dy * dz + dz * dx;
            if (area > best_area) { best_area = area; best = c; }
        }
        if (best < 0) break;
        const int2 ch = children[cand[best]];
        cand[best] = ch.x; cand[ncand++] = ch.y;
    }
    Bvh4Node out;
    for (int c = 0; c < 4; ++c) {
        if (c < ncand) {
            const float* b = cand[c] >= 0 ? node_box + 6 * (size_t)cand[c] : leaf_box + 6 * (size_t)(~cand[c]);
            out.lox[c] = b[0]; out.loy[c] = b[1]; out.loz[c] = b[2]; out.hix[c] = b[3]; out.hiy[c] = b[4]; out.hiz[c] = b[5];
            out.child[c] = cand[c] >= 0 ? new_id[cand[c]] : cand[c];
        } else {
            out.lox[c] = out.loy[c] = out.loz[c] = __builtin_huge_valf();
            out.hix[c] = out.hiy[c] = out.hiz[c] = -__builtin_huge_valf();
            out.child[c] = 0x7FFFFFFF;
        }
        out.pad[c] = 0;
    }
    nodes4[(size_t)new_id[i]] = out;
}

// shader/extract_tri_lights.comp:17-54 (all emissive instances in one launch)
__global__ __launch_bounds__(BT) void k_extract_tri_lights(SceneView sv, const uint* tri_prefix, TriLight* out) {
    uint gid = blockIdx.x * BT + threadIdx.x;
    if (gid >= sv.tri_count) return;
    uint inst, prim;
    locate_triangle(tri_prefix, sv.instance_count, gid, inst, prim);
    const Instance& o = sv.instances[inst];
    if (o.light_base_id < 0) return;
    const MeshSpan sp = sv.spans[inst];
    const uint* ix = sv.indices + sp.index_offset + 3u * prim;
    const Vertex* vb = sv.vertices + sp.vertex_offset;
    const Vertex v0 = vb[ix[0]], v1 = vb[ix[1]], v2 = vb[ix[2]];
    TriLight l;
    l.emission_tex_id = o.mat.emission_tex_id;
    l.emission_factor = rgb_to_r9g9b9e5(F3(o.mat.emission_factor));
    l.instance_id = inst;
    l.primitive_id = prim;
    l.pos[0] = transform_point(o.model, v0.pos);
    l.pos[1] = transform_point(o.model, v1.pos);
    l.pos[2] = transform_point(o.model, v2.pos);
    l.uv[0] = pack_half2x16(v0.uv); l.uv[1] = pack_half2x16(v1.uv); l.uv[2] = pack_half2x16(v2.uv);
    out[(uint)o.light_base_id + prim] = l;
}

// The emitter set of the terminal query (common.h EmitterSet), from the records the tree's leaves hold: which of
// them belong to an instance that emits (or that tri-light sampling knows, whatever its emission), ...
__global__ __launch_bounds__(BT) void k_emitter_gather(const Instance* instances, const TriRecord* tris, uint n, EmitterSet* es) {
    const uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    const Instance& o = instances[tris[i].inst_flags & 0x7FFFFFFFu];
    const f4 e = o.mat.emission_factor;
    if (!(e.x != 0.0f || e.y != 0.0f || e.z != 0.0f || o.light_base_id >= 0)) return;
    const uint slot = atomicAdd(&es->count, 1u);
    if (slot < TR_EMITTER_MAX) es->index[slot] = i;
}
// ... then, one thread: the list in ascending order and the union box of its triangles (exact minima and maxima of the records' vertices)
__global__ void k_emitter_finish(const TriRecord* tris, EmitterSet* es) {
    const uint c = es->count <= TR_EMITTER_MAX ? es->count : 0u;      // above the threshold the query does not run: an empty box
    for (uint a = 1; a < c; ++a) {
        const uint v = es->index[a];
        uint b = a;
        for (; b > 0 && es->index[b - 1] > v; --b) es->index[b] = es->index[b - 1];
        es->index[b] = v;
    }
    float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()}, hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    for (uint a = 0; a < c; ++a) {
        const TriRecord& t = tris[es->index[a]];
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(fminf(lo[k], t.v0[k]), fminf(t.v1[k], t.v2[k]));
            hi[k] = fmaxf(fmaxf(hi[k], t.v0[k]), fmaxf(t.v1[k], t.v2[k]));
        }
    }
    for (int k = 0; k < 3; ++k)
        for (int slot = 0; slot < 4; ++slot) {      // a Bvh4Node's planes: lo of axis k at 8 k, hi at 8 k + 4; the box sits in slot 0
            es->planes[8 * k + slot] = slot == 0 ? lo[k] : __builtin_huge_valf();
            es->planes[8 * k + 4 + slot] = slot == 0 ? hi[k] : -__builtin_huge_valf();
        }
}

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return set_error(std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

}  // namespace

// shader/pre_transform.comp:26-42
__global__ __launch_bounds__(BT) void k_pre_transform_vertices(uint vertex_count, const Instance* instance, const Vertex* in, Vertex* out) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= vertex_count) return;
    const m4 model = instance->model;
    const m3 mn = upper3(instance->model_normal);
    // determinant(mat3(o.model_normal)), cofactor expansion along the first column
    const float det = mn.c[0].x * (mn.c[1].y * mn.c[2].z - mn.c[2].y * mn.c[1].z)
                    - mn.c[1].x * (mn.c[0].y * mn.c[2].z - mn.c[2].y * mn.c[0].z)
                    + mn.c[2].x * (mn.c[0].y * mn.c[1].z - mn.c[1].y * mn.c[0].z);
    Vertex v = in[i];
    v.pos = transform_point(model, v.pos);
    v.normal = normalize(mul(mn, v.normal));
    f3 t = normalize(mul(mn, F3(v.tangent)));
    v.tangent = F4(t, v.tangent.w);
    if (det < 0) { v.normal = -v.normal; v.tangent = F4(-t.x, -t.y, -t.z, -v.tangent.w); }
    out[i] = v;
}

// After a build or a refit of the all-merged structure (an instance update makes one of the two necessary, so a changed material is seen)
static int gather_emitters(DeviceScene& ds, hipStream_t stream) {
    ds.emitter_count = 0xFFFFFFFFu;
    if (!ds.tris || ds.leaf_count != ds.tri_count) return 0;
    EmitterSet* es = reinterpret_cast<EmitterSet*>(ds.tris + ds.tri_count);
    HIPCHK(hipMemsetAsync(es, 0, sizeof(EmitterSet), stream));
    hipLaunchKernelGGL(k_emitter_gather, dim3((ds.tri_count + BT - 1) / BT), dim3(BT), 0, stream, ds.instances, ds.tris, ds.tri_count, es);
    hipLaunchKernelGGL(k_emitter_finish, dim3(1), dim3(1), 0, stream, ds.tris, es);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&ds.emitter_count, &es->count, sizeof(uint), hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
}

int ensure_world_vertices(DeviceScene& ds, hipStream_t stream) {
    if (ds.world_vertices || ds.world_vertex_count == 0) return 0;
    HIPCHK(hipMalloc(&ds.world_vertices, (size_t)ds.world_vertex_count * sizeof(Vertex)));
    for (uint i = 0; i < ds.instance_count; ++i) {   // one dispatch per instance, as src/scene_stage.cc:1685-1723 records them
        const MeshSpan& sp = ds.host_spans[i];
        if (sp.vertex_count == 0) continue;
        hipLaunchKernelGGL(k_pre_transform_vertices, dim3((sp.vertex_count + BT - 1) / BT), dim3(BT), 0, stream, sp.vertex_count, ds.instances + i,
                           ds.vertices + sp.vertex_offset, ds.world_vertices + ds.host_world_spans[i].vertex_offset);
    }
    HIPCHK(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// shader/skinning.comp:44-71, dispatched per skinned mesh by scene_stage::record_skinning (src/scene_stage.cc:1543-1567).
// skin_mat = sum w_k * joint[k]; positions go through skin_mat, normals and tangents through transpose(inverse(skin_mat)).
// GLSL leaves the arithmetic of inverse() to the driver; here it is the cofactor expansion over 2x2 sub-determinants
// (only the upper-left 3x3 of the inverse reaches a direction), identical in oracle/oracle.cc so results match bit for bit.
// The previous-position buffer the shader also fills is read by the raster path only (shader/forward.vert:28); here the previous
// positions are kept by k_latch_positions (below), once per frame and ahead of this kernel, when trhip_scene_set_deformation_motion is on.
__global__ __launch_bounds__(BT) void k_skinning(uint vertex_count, const Vertex* source, const Skin* skins, const m4* joints, uint joint_count, Vertex* destination) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= vertex_count) return;
    const Skin s = skins[i];
    float a[4][4];   // a[r][c]
    for (int c = 0; c < 4; ++c) {
        f4 col = F4(0);
        for (int k = 0; k < 4; ++k) {
            const uint j = s.joints[k] < joint_count ? s.joints[k] : 0u;   // out-of-range joint ids are undefined behaviour in the shader
            const f4 t = joints[j].c[c] * s.weights[k];
            col = k == 0 ? t : col + t;
        }
        a[0][c] = col.x; a[1][c] = col.y; a[2][c] = col.z; a[3][c] = col.w;
    }
    const float s0 = a[0][0] * a[1][1] - a[1][0] * a[0][1], s1 = a[0][0] * a[1][2] - a[1][0] * a[0][2], s2 = a[0][0] * a[1][3] - a[1][0] * a[0][3];
    const float s3 = a[0][1] * a[1][2] - a[1][1] * a[0][2], s4 = a[0][1] * a[1][3] - a[1][1] * a[0][3], s5 = a[0][2] * a[1][3] - a[1][2] * a[0][3];
    const float c5 = a[2][2] * a[3][3] - a[3][2] * a[2][3], c4 = a[2][1] * a[3][3] - a[3][1] * a[2][3], c3 = a[2][1] * a[3][2] - a[3][1] * a[2][2];
    const float c2 = a[2][0] * a[3][3] - a[3][0] * a[2][3], c1 = a[2][0] * a[3][2] - a[3][0] * a[2][2], c0 = a[2][0] * a[3][1] - a[3][0] * a[2][1];
    const float det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    float inv[3][3];   // inv[r][c], upper-left block of inverse(skin_mat)
    inv[0][0] = ( a[1][1] * c5 - a[1][2] * c4 + a[1][3] * c3) / det;
    inv[0][1] = (-a[0][1] * c5 + a[0][2] * c4 - a[0][3] * c3) / det;
    inv[0][2] = ( a[3][1] * s5 - a[3][2] * s4 + a[3][3] * s3) / det;
    inv[1][0] = (-a[1][0] * c5 + a[1][2] * c2 - a[1][3] * c1) / det;
    inv[1][1] = ( a[0][0] * c5 - a[0][2] * c2 + a[0][3] * c1) / det;
    inv[1][2] = (-a[3][0] * s5 + a[3][2] * s2 - a[3][3] * s1) / det;
    inv[2][0] = ( a[1][0] * c4 - a[1][1] * c2 + a[1][3] * c0) / det;
    inv[2][1] = (-a[0][0] * c4 + a[0][1] * c2 - a[0][3] * c0) / det;
    inv[2][2] = ( a[3][0] * s4 - a[3][1] * s2 + a[3][3] * s0) / det;
    const Vertex src = source[i];
    Vertex dst = src;
    dst.pos = F3(a[0][0] * src.pos.x + a[0][1] * src.pos.y + a[0][2] * src.pos.z + a[0][3],
                 a[1][0] * src.pos.x + a[1][1] * src.pos.y + a[1][2] * src.pos.z + a[1][3],
                 a[2][0] * src.pos.x + a[2][1] * src.pos.y + a[2][2] * src.pos.z + a[2][3]);
    // transpose(inverse(M)) * (d, 0): component r = sum_c inv[c][r] * d_c
    const f3 n = src.normal, t = F3(src.tangent);
    // (the w = 0 column of the 4x4 product contributes +0: keeps the sign of a zero component as GLSL has it)
    dst.normal = normalize(F3(inv[0][0] * n.x + inv[1][0] * n.y + inv[2][0] * n.z + 0.0f, inv[0][1] * n.x + inv[1][1] * n.y + inv[2][1] * n.z + 0.0f,
                              inv[0][2] * n.x + inv[1][2] * n.y + inv[2][2] * n.z + 0.0f));
    const f3 tt = normalize(F3(inv[0][0] * t.x + inv[1][0] * t.y + inv[2][0] * t.z + 0.0f, inv[0][1] * t.x + inv[1][1] * t.y + inv[2][1] * t.z + 0.0f,
                               inv[0][2] * t.x + inv[1][2] * t.y + inv[2][2] * t.z + 0.0f));
    dst.tangent = F4(tt, src.tangent.w);
    destination[i] = dst;
}

// glTF morph targets ahead of skinning: morph.h pins the order of operations (tests/morph_model.py repeats it bit for bit).  One lane per
// vertex; the active list is the same for every lane (a uniform trip count), and lane i reads floats 3 i .. 3 i + 2 of an active target's
// plane, so a wave reads 768 consecutive bytes per plane and target.  No atomics: two runs give the same bits.  Like k_skinning it writes
// no previous positions: k_latch_positions keeps them.
__device__ inline f3 morph_accumulate(f3 acc, const float* plane, size_t vertex_count, uint i, const MorphActive* active, uint active_count) {
    for (uint a = 0; a < active_count; ++a) {
        const MorphActive m = active[a];
        const float* d = plane + ((size_t)m.index * vertex_count + i) * 3u;
        acc.x = acc.x + m.weight * d[0];      // two roundings each: the build has contraction off (Makefile)
        acc.y = acc.y + m.weight * d[1];
        acc.z = acc.z + m.weight * d[2];
    }
    return acc;
}
__device__ inline f3 morph_direction(f3 acc, f3 base) {
    const float d = (acc.x * acc.x + acc.y * acc.y) + acc.z * acc.z;
    const float len = sqrtf(d);      // sqrtf and / are correctly rounded in this build (the device library's intrinsic __fsqrt_rn is not)
    return len > 0.0f ? F3(acc.x / len, acc.y / len, acc.z / len) : base;
}
__global__ __launch_bounds__(BT) void k_morph(uint vertex_count, const Vertex* base, const float* dpos, const float* dnrm, const float* dtan,
                                              const MorphActive* active, uint active_count, Vertex* destination) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= vertex_count) return;
    const Vertex src = base[i];
    Vertex dst = src;
    if (active_count) {
        dst.pos = morph_accumulate(src.pos, dpos, vertex_count, i, active, active_count);
        if (dnrm) dst.normal = morph_direction(morph_accumulate(src.normal, dnrm, vertex_count, i, active, active_count), src.normal);
        if (dtan) {
            const f3 t = F3(src.tangent);
            dst.tangent = F4(morph_direction(morph_accumulate(t, dtan, vertex_count, i, active, active_count), t), src.tangent.w);
        }
    }
    destination[i] = dst;
}

// The previous positions of deforming meshes (trhip_scene_latch_positions): the positions of the listed spans as
// they stand in the scene go to the plane surface_prev_pos reads (shading.h), float[vertex][3] parallel to the vertex array.  blockIdx.y
// names the span, one lane per vertex; a lane reads the 12 bytes of a 48-byte vertex that are its position and writes 12 packed bytes,
// so a wave writes 768 consecutive bytes.  Blocks past the end of a span shorter than the longest leave at once.  No atomics, no LDS.
// Bounds: `spans` holds gridDim.y records whose vertex_offset + vertex_count the upload checked against the vertex array, and the plane
// has a slot per vertex of that array.
__global__ __launch_bounds__(BT) void k_latch_positions(const MeshSpan* spans, const Vertex* vertices, float* previous) {
    const MeshSpan sp = spans[blockIdx.y];
    const uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= sp.vertex_count) return;
    const size_t v = (size_t)sp.vertex_offset + i;
    const f3 p = vertices[v].pos;
    float* out = previous + 3u * v;
    out[0] = p.x; out[1] = p.y; out[2] = p.z;
}

__global__ __launch_bounds__(BT) void k_build_shade_tris(uint n_spans, const MeshSpan* spans, const Vertex* vertices, const uint* indices, ShadeTri* out, f4* tangents) {
    const MeshSpan sp = spans[blockIdx.y];
    const Vertex* vb = vertices + sp.vertex_offset;
    const uint* ix = indices + sp.index_offset;
    ShadeTri* o = out + sp.index_offset / 3u;
    f4* ot = tangents + (size_t)sp.index_offset;      // three per record: index_offset / 3 * 3
    for (uint t = blockIdx.x * BT + threadIdx.x; t < sp.triangle_count; t += gridDim.x * BT) {
        ShadeTri r;
        for (int k = 0; k < 3; ++k) {
            const Vertex v = vb[ix[3 * t + k]];
            r.pos[k] = v.pos; r.normal[k] = v.normal; r.uv[k] = v.uv;
            ot[3 * t + k] = v.tangent;
        }
        for (float& x : r.pad) x = 0.0f;
        o[t] = r;
    }
}

// The per-triangle vertex records k_shade reads (common.h ShadeTri).  A record is addressed by index_offset / 3 + primitive, so every
// span must start at a whole triangle and two spans over the same indices must use the same vertices; a scene that does not
// (none the loaders produce) simply has no records and is shaded by the general kernels.
int build_shade_tris(DeviceScene& ds, int instance, hipStream_t stream) {
    if (instance < 0) {
        if (ds.shade_tris) { (void)hipFree(ds.shade_tris); ds.shade_tris = nullptr; ds.shade_tangents = nullptr; }
        if (ds.index_count < 3 || ds.instance_count == 0 || getenv("TRHIP_NO_SHADE_TRIS")) return 0;
        std::vector<MeshSpan> unique;
        {
            std::vector<MeshSpan> sorted(ds.host_spans);
            std::sort(sorted.begin(), sorted.end(), [](const MeshSpan& a, const MeshSpan& b) { return a.index_offset != b.index_offset ? a.index_offset < b.index_offset : a.triangle_count > b.triangle_count; });
            uint64_t end = 0;      // first index not covered by the records so far
            for (const MeshSpan& sp : sorted) {
                if (sp.triangle_count == 0) continue;
                if (sp.index_offset % 3u != 0) return 0;
                if (!unique.empty() && sp.index_offset < end) {      // overlaps the previous mesh: fine if it is (part of) the same mesh
                    const MeshSpan& u = unique.back();
                    if (sp.vertex_offset != u.vertex_offset || (sp.index_offset - u.index_offset) % 3u != 0 || (uint64_t)sp.index_offset + 3ull * sp.triangle_count > end) return 0;
                    continue;
                }
                unique.push_back(sp);
                end = (uint64_t)sp.index_offset + 3ull * sp.triangle_count;
            }
        }
        if (unique.empty()) return 0;
        {   // records, then the tangents (three f4 per record) in the same allocation
            const size_t n_rec = ds.index_count / 3u;
            HIPCHK(hipMalloc(&ds.shade_tris, n_rec * (sizeof(ShadeTri) + 3 * sizeof(f4))));
            ds.shade_tangents = reinterpret_cast<f4*>(ds.shade_tris + n_rec);
        }
        MeshSpan* dev_spans = nullptr;
        HIPCHK(hipMalloc(&dev_spans, unique.size() * sizeof(MeshSpan)));
        HIPCHK(hipMemcpyAsync(dev_spans, unique.data(), unique.size() * sizeof(MeshSpan), hipMemcpyHostToDevice, stream));
        uint most = 0;
        for (const MeshSpan& sp : unique) most = std::max(most, sp.triangle_count);
        for (size_t first = 0; first < unique.size(); first += 65535u) {
            const uint count = (uint)std::min<size_t>(65535u, unique.size() - first);
            hipLaunchKernelGGL(k_build_shade_tris, dim3(std::min((most + BT - 1) / BT, 1024u), count), dim3(BT), 0, stream, count, dev_spans + first, ds.vertices, ds.indices, ds.shade_tris, ds.shade_tangents);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(stream));
        (void)hipFree(dev_spans);
        return 0;
    }
    if (!ds.shade_tris) return 0;
    // one mesh again (its vertices were skinned): the span of the instance, read from the device copy of the spans
    const MeshSpan& sp = ds.host_spans[(size_t)instance];
    if (sp.triangle_count == 0) return 0;
    hipLaunchKernelGGL(k_build_shade_tris, dim3(std::min((sp.triangle_count + BT - 1) / BT, 1024u), 1), dim3(BT), 0, stream, 1u, ds.spans + instance, ds.vertices, ds.indices, ds.shade_tris, ds.shade_tangents);
    HIPCHK(hipGetLastError());
    return 0;
}

int skin_instance(DeviceScene& ds, uint instance, const float* joint_transforms, uint joint_count, hipStream_t stream) {
    if (instance >= ds.skin_slots.size() || !ds.skin_slots[instance].source) return set_error("trhip_scene_skin: instance has no skin (trhip_scene_set_skin)");
    DeviceScene::SkinSlot& k = ds.skin_slots[instance];
    if (joint_count == 0 || !joint_transforms) return set_error("trhip_scene_skin: no joint transforms");
    if (joint_count > k.joint_capacity) {
        if (k.joints) (void)hipFree(k.joints);
        k.joints = nullptr; k.joint_capacity = 0;
        HIPCHK(hipMalloc(&k.joints, (size_t)joint_count * sizeof(m4)));
        k.joint_capacity = joint_count;
    }
    HIPCHK(hipMemcpyAsync(k.joints, joint_transforms, (size_t)joint_count * sizeof(m4), hipMemcpyHostToDevice, stream));
    const MeshSpan& sp = ds.host_spans[instance];
    hipLaunchKernelGGL(k_skinning, dim3((k.vertex_count + BT - 1) / BT), dim3(BT), 0, stream, k.vertex_count, k.source, k.skins, k.joints, joint_count,
                       ds.vertices + sp.vertex_offset);
    HIPCHK(hipGetLastError());
    if (int rc = build_shade_tris(ds, (int)instance, stream)) return rc;
    HIPCHK(hipStreamSynchronize(stream));   // the host array may be reused by the caller
    return 0;
}

// trhip_scene_morph behind its argument checks: compacts the non-zero weights into the slot's active list (grown like SkinSlot::joints) and
// runs k_morph from the slot's base into the skin slot's source (glTF morphs before it skins: the scene's vertices change at the next
// trhip_scene_skin) or, on an instance without a skin, into the instance's vertex span, followed by the shade-triangle rebuild of skin_instance.
int morph_instance(DeviceScene& ds, uint instance, const float* weights, uint weight_count, hipStream_t stream) {
    DeviceScene::MorphSlot& m = ds.morph_slots[instance];
    std::vector<MorphActive> active;
    for (uint k = 0; k < weight_count; ++k) if (weights[k] != 0.0f) active.push_back(MorphActive{k, weights[k]});
    if (active.size() > m.active_capacity) {
        if (m.active) (void)hipFree(m.active);
        m.active = nullptr; m.active_capacity = 0;
        HIPCHK(hipMalloc(&m.active, active.size() * sizeof(MorphActive)));
        m.active_capacity = (uint)active.size();
    }
    if (!active.empty()) HIPCHK(hipMemcpyAsync(m.active, active.data(), active.size() * sizeof(MorphActive), hipMemcpyHostToDevice, stream));
    const bool skinned = instance < ds.skin_slots.size() && ds.skin_slots[instance].source;
    const MeshSpan& sp = ds.host_spans[instance];
    Vertex* destination = skinned ? ds.skin_slots[instance].source : ds.vertices + sp.vertex_offset;
    if (m.vertex_count) {
        hipLaunchKernelGGL(k_morph, dim3((m.vertex_count + BT - 1) / BT), dim3(BT), 0, stream, m.vertex_count, m.base, m.dpos, m.dnrm, m.dtan, m.active,
                           (uint)active.size(), destination);
        HIPCHK(hipGetLastError());
    }
    if (!skinned) if (int rc = build_shade_tris(ds, (int)instance, stream)) return rc;
    HIPCHK(hipStreamSynchronize(stream));   // `active` leaves scope
    return 0;
}

// The device list of k_latch_positions: record 0 is the whole vertex array (what the fill copies), behind it every vertex range that a
// skin or morph targets deform, once (instances that share a span move together; a morphed and skinned instance is its span, the
// skinned result).  Rebuilt when a skin or targets were set since the last time.
static int update_latch_spans(DeviceScene& ds, hipStream_t stream) {
    if (ds.latch_spans_valid) return 0;
    std::vector<MeshSpan> list(1, MeshSpan{0u, ds.vertex_count, 0u, 0u});
    std::vector<std::pair<uint, uint>> seen;
    uint most = 0;
    for (uint i = 0; i < ds.instance_count; ++i) {
        if (!((i < ds.skin_slots.size() && ds.skin_slots[i].source) || ds.has_morph(i))) continue;
        const MeshSpan& sp = ds.host_spans[i];
        const std::pair<uint, uint> range(sp.vertex_offset, sp.vertex_count);
        if (sp.vertex_count == 0 || std::find(seen.begin(), seen.end(), range) != seen.end()) continue;
        seen.push_back(range);
        list.push_back(MeshSpan{sp.vertex_offset, sp.vertex_count, 0u, 0u});
        most = std::max(most, sp.vertex_count);
    }
    if (ds.latch_spans) { (void)hipFree(ds.latch_spans); ds.latch_spans = nullptr; }
    ds.latch_span_count = 0; ds.latch_span_most = 0;
    HIPCHK(hipMalloc(&ds.latch_spans, list.size() * sizeof(MeshSpan)));
    HIPCHK(hipMemcpyAsync(ds.latch_spans, list.data(), list.size() * sizeof(MeshSpan), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));   // `list` leaves scope
    ds.latch_span_count = (uint)list.size() - 1u;
    ds.latch_span_most = most;
    ds.latch_spans_valid = true;
    return 0;
}

int fill_previous_positions(DeviceScene& ds, hipStream_t stream) {
    ds.free_previous_positions();
    if (ds.vertex_count == 0 || !ds.vertices) return 0;      // nothing to keep: surface_prev_pos is never reached either
    HIPCHK(hipMalloc(&ds.prev_positions, (size_t)ds.vertex_count * 3u * sizeof(float)));
    if (int rc = update_latch_spans(ds, stream)) return rc;
    hipLaunchKernelGGL(k_latch_positions, dim3((ds.vertex_count + BT - 1) / BT, 1), dim3(BT), 0, stream, ds.latch_spans, ds.vertices, ds.prev_positions);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
}

int latch_positions(DeviceScene& ds, hipStream_t stream) {
    if (!ds.prev_positions) return 0;
    if (int rc = update_latch_spans(ds, stream)) return rc;
    if (ds.latch_span_count == 0) return 0;      // the listed spans are not empty
    for (uint first = 0; first < ds.latch_span_count; first += 65535u) {      // gridDim.y is 16 bits wide
        const uint count = std::min(65535u, ds.latch_span_count - first);
        hipLaunchKernelGGL(k_latch_positions, dim3((ds.latch_span_most + BT - 1) / BT, count), dim3(BT), 0, stream, ds.latch_spans + 1 + first, ds.vertices, ds.prev_positions);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(stream));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// Refit: the instance transforms changed, the tree keeps its topology (what a BLAS/TLAS *update* does in the reference,
// src/acceleration_structure.cc:376-422).  World triangles are recomputed in place, then the child boxes of the live
// nodes are rebuilt level by level from the deepest level up.
__global__ __launch_bounds__(BT) void k_retransform(SceneView sv, uint n, TriRecord* tris, const uint* alpha_base, AlphaTri* alpha_tris) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    TriRecord t = tris[i];
    const uint inst = t.inst_flags & 0x7FFFFFFFu;
    const MeshSpan sp = sv.obj_spans[inst];
    const uint* ix = sv.indices + sp.index_offset + 3u * t.prim;
    const Vertex* vb = sv.obj_vertices + sp.vertex_offset;
    const m4 model = sv.instances[inst].model;
    const f3 p0 = transform_point(model, vb[ix[0]].pos), p1 = transform_point(model, vb[ix[1]].pos), p2 = transform_point(model, vb[ix[2]].pos);
    t.v0[0] = p0.x; t.v0[1] = p0.y; t.v0[2] = p0.z;
    t.v1[0] = p1.x; t.v1[1] = p1.y; t.v1[2] = p1.z;
    t.v2[0] = p2.x; t.v2[1] = p2.y; t.v2[2] = p2.z;
    if (t.inst_flags & 0x80000000u) t.alpha = alpha_word(sv.instances[inst].mat, alpha_base[inst] + t.prim, alpha_tris, vb[ix[0]].uv, vb[ix[1]].uv, vb[ix[2]].uv);
    tris[i] = t;
}

// breadth-first expansion of one level of live nodes (run once per build, on the first refit)
__global__ __launch_bounds__(BT) void k_expand_level(uint count, const uint* level, const Bvh4Node* nodes4, uint* next, uint* next_count) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= count) return;
    const Bvh4Node& nd = nodes4[level[i]];
    for (int c = 0; c < 4; ++c) {
        const int ch = nd.child[c];
        if (ch >= 0 && ch != 0x7FFFFFFF) next[atomicAdd(next_count, 1u)] = (uint)ch;
    }
}

__global__ __launch_bounds__(BT) void k_refit_level(uint count, const uint* level, Bvh4Node* nodes4, const TriRecord* tris, float* node_bounds) {
    uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= count) return;
    const uint id = level[i];
    Bvh4Node nd = nodes4[id];
    float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    for (int c = 0; c < 4; ++c) {
        const int ch = nd.child[c];
        if (ch == 0x7FFFFFFF) continue;
        float blo[3], bhi[3];
        if (ch < 0) {
            const TriRecord& t = tris[~ch];
            for (int k = 0; k < 3; ++k) { blo[k] = fminf(fminf(t.v0[k], t.v1[k]), t.v2[k]); bhi[k] = fmaxf(fmaxf(t.v0[k], t.v1[k]), t.v2[k]); }
        } else {
            for (int k = 0; k < 3; ++k) { blo[k] = node_bounds[6 * (size_t)ch + k]; bhi[k] = node_bounds[6 * (size_t)ch + 3 + k]; }
        }
        nd.lox[c] = blo[0]; nd.loy[c] = blo[1]; nd.loz[c] = blo[2]; nd.hix[c] = bhi[0]; nd.hiy[c] = bhi[1]; nd.hiz[c] = bhi[2];
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], blo[k]); hi[k] = fmaxf(hi[k], bhi[k]); }
    }
    nodes4[id] = nd;
    for (int k = 0; k < 3; ++k) { node_bounds[6 * (size_t)id + k] = lo[k]; node_bounds[6 * (size_t)id + 3 + k] = hi[k]; }
}

static int refit_two_level(DeviceScene& ds, hipStream_t stream, trhip_accel_info* info);
int refit_accel(DeviceScene& ds, hipStream_t stream, trhip_accel_info* info) {
    if (ds.two_level) {
        if (ds.accel_tri_count != ds.tri_count || ds.tlas_capacity != ds.tlas_leaf_count)
            return set_error("trhip_scene_refit_accel: no acceleration structure to refit; call trhip_scene_build_accel first");
        return refit_two_level(ds, stream, info);
    }
    const uint n = ds.leaf_count;      // records in ds.tris: triangles, or the references of a pre-split build (their leaf boxes grow to the whole triangle here)
    if (ds.accel_tri_count != ds.tri_count || ds.accel_capacity == 0xFFFFFFFFu || (n > 0 && !ds.tris) || (n > 1 && !ds.nodes4))
        return set_error("trhip_scene_refit_accel: no acceleration structure to refit; call trhip_scene_build_accel first");
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, stream));
    SceneView sv = ds.view();
    const uint n1 = ds.node_count;
    if (n1 > 0 && !ds.levels_valid) {   // once per build: live nodes by level
        if (!ds.level_nodes) HIPCHK(hipMalloc(&ds.level_nodes, (size_t)n1 * 4));
        if (!ds.node_bounds) HIPCHK(hipMalloc(&ds.node_bounds, (size_t)n1 * 24));
        uint* counter = nullptr;
        HIPCHK(hipMalloc(&counter, 4));
        const uint root = 0;
        HIPCHK(hipMemcpyAsync(ds.level_nodes, &root, 4, hipMemcpyHostToDevice, stream));
        ds.level_offsets.assign(1, 0u);
        uint begin = 0, count = 1;
        while (count > 0) {
            ds.level_offsets.push_back(begin + count);
            if (begin + count >= n1) break;   // all node slots used: nothing can follow
            HIPCHK(hipMemsetAsync(counter, 0, 4, stream));
            hipLaunchKernelGGL(k_expand_level, dim3((count + BT - 1) / BT), dim3(BT), 0, stream, count, ds.level_nodes + begin, ds.nodes4,
                               ds.level_nodes + begin + count, counter);
            uint next = 0;
            HIPCHK(hipMemcpyAsync(&next, counter, 4, hipMemcpyDeviceToHost, stream));
            HIPCHK(hipStreamSynchronize(stream));
            begin += count; count = next;
            if (ds.level_offsets.size() > 4096) { (void)hipFree(counter); return set_error("trhip_scene_refit_accel: hierarchy too deep"); }
        }
        (void)hipFree(counter);
        ds.levels_valid = true;
        if (getenv("TRHIP_DEBUG"))
            fprintf(stderr, "[trhip] 4-wide tree: %u live nodes of %u slots in %zu levels, %.3f children per node\n", ds.level_offsets.back(), n1,
                    ds.level_offsets.size() - 1, (double)(n + ds.level_offsets.back() - 1) / (double)ds.level_offsets.back());
    }
    if (n > 0) hipLaunchKernelGGL(k_retransform, dim3((n + BT - 1) / BT), dim3(BT), 0, stream, sv, n, ds.tris, ds.alpha_base, ds.alpha_tris);
    for (size_t l = ds.level_offsets.size(); l-- > 1;) {
        const uint lo = ds.level_offsets[l - 1], cnt = ds.level_offsets[l] - lo;
        if (cnt) hipLaunchKernelGGL(k_refit_level, dim3((cnt + BT - 1) / BT), dim3(BT), 0, stream, cnt, ds.level_nodes + lo, ds.nodes4, ds.tris, ds.node_bounds);
    }
    HIPCHK(hipGetLastError());
    ds.accel_built = true;
    if (ds.gather_emissive_triangles && ds.host_tri_light_count > 0 && ds.tri_lights) {
        HIPCHK(hipMemsetAsync(ds.tri_lights, 0, (size_t)ds.host_tri_light_count * sizeof(TriLight), stream));
        SceneView sv2 = ds.view();
        hipLaunchKernelGGL(k_extract_tri_lights, dim3((ds.tri_count + BT - 1) / BT), dim3(BT), 0, stream, sv2, ds.tri_prefix, ds.tri_lights);
    }
    if (int rc = gather_emitters(ds, stream)) return rc;
    HIPCHK(hipEventRecord(e1, stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    ds.layout.blas_updated = 1; ds.layout.blas_ms = ms;
    if (info) {
        memset(info, 0, sizeof(*info));
        info->triangle_count = ds.tri_count; info->leaf_count = n; info->node_count = ds.node_count; info->node_bytes = 112u; info->tri_light_count = ds.tri_light_count;
        info->build_ms = ms;
        for (int k = 0; k < 3; ++k) { info->bounds_min[k] = ds.bounds_lo[k]; info->bounds_max[k] = ds.bounds_hi[k]; }
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// One tree over n records: the scratch plan (sized for up to n_cap leaves; the arena survives the call) and the pipeline from the
// unsorted records + their centroid bounds to sorted records and 4-wide nodes.  trhip_scene_build_accel runs it once over every world
// triangle (all-merged); the two-level build once per BLAS and once over the instance boxes of the TLAS.
struct TreePlan {
    size_t sort_bytes = 0, scan_bytes = 0;
    size_t o_cbounds, o_unsorted, o_keys, o_keys_sorted, o_vals, o_vals_sorted, o_leaf_box, o_sort, o_children, o_sizes, o_parent, o_parent_leaf,
           o_node_box, o_arrive, o_cref0, o_cref1, o_cbox0, o_cbox1, o_nn, o_valid, o_pos, o_scan, o_new_id, o_nodes2;
    size_t o_uparent, o_moves, o_lock, o_optstat, o_ccost, o_cdec;
    char* base = nullptr;
    uint* cbounds() const { return reinterpret_cast<uint*>(base + o_cbounds); }   // 6 flipped centroid bounds, [6] PLOC node allocator, [8..9] cluster counts
    TriRecord* unsorted() const { return reinterpret_cast<TriRecord*>(base + o_unsorted); }
};

static int plan_tree(DeviceScene& ds, hipStream_t stream, uint n_cap, TreePlan& P) {
    size_t& sort_bytes = P.sort_bytes;
    size_t& scan_bytes = P.scan_bytes;
    const uint n_tri = n_cap;
    size_t plan_bytes = 0;
    auto plan = [&](size_t bytes) { size_t o = plan_bytes; plan_bytes += (bytes + 255) & ~(size_t)255; return o; };
    const size_t n1 = n_cap > 1 ? n_cap - 1 : 0;     // inner nodes the buffers hold
    if (n_cap > 0) {
        HIPCHK(rocprim::radix_sort_pairs(nullptr, sort_bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (uint*)nullptr, (uint*)nullptr, n_cap, 0, 64, stream));
        HIPCHK(rocprim::exclusive_scan(nullptr, scan_bytes, (uint*)nullptr, (uint*)nullptr, 0u, n_cap + BT, rocprim::plus<uint>(), stream));
    }
    P.o_cbounds = plan(32 * sizeof(uint)); P.o_unsorted = plan((size_t)n_cap * sizeof(TriRecord)); P.o_keys = plan((size_t)n_cap * 8);
    P.o_keys_sorted = plan((size_t)n_cap * 8); P.o_vals = plan((size_t)n_cap * 4); P.o_vals_sorted = plan((size_t)n_cap * 4);
    P.o_leaf_box = plan((size_t)n_cap * 24); P.o_sort = plan(sort_bytes + 16); P.o_children = plan(n1 * sizeof(int2));
    P.o_sizes = plan(n1 * 4); P.o_parent = plan(n1 * 4); P.o_parent_leaf = plan((size_t)n_cap * 4); P.o_node_box = plan(n1 * 24);
    P.o_arrive = plan(n1 * 4); P.o_cref0 = plan((size_t)n_cap * 4); P.o_cref1 = plan((size_t)n_cap * 4);
    P.o_cbox0 = plan((size_t)n_cap * 24); P.o_cbox1 = plan((size_t)n_cap * 24); P.o_nn = plan((size_t)n_cap * 4);
    P.o_valid = plan(((size_t)n_cap + BT) * 4); P.o_pos = plan(((size_t)n_cap + BT) * 4); P.o_scan = plan(scan_bytes + 16);
    P.o_new_id = plan(n1 * 4); P.o_nodes2 = plan(n1 * sizeof(BvhNode));
    const bool optimise = ds.optimise_rounds > 0 && !ds.fast_build && n_tri > 2;
    const size_t n_all_cap = (size_t)n_cap + n1;
    const bool dp_collapse = ds.collapse_by_cost && !ds.fast_build && n_tri > 2;   // a fast build keeps the greedy choice (the cost pass would double its time)
    P.o_uparent = plan(optimise || dp_collapse ? n_all_cap * 4 : 0); P.o_moves = plan(optimise ? n_all_cap * sizeof(OptMove) : 0);
    P.o_lock = plan(optimise ? n_all_cap * 8 : 0); P.o_optstat = plan(64); P.o_ccost = plan(dp_collapse ? n1 * 12 : 0);
    P.o_cdec = plan(dp_collapse ? n1 : 0);
    if (plan_bytes > ds.scratch_bytes) {
        if (ds.scratch) (void)hipFree(ds.scratch);
        ds.scratch = nullptr; ds.scratch_bytes = 0;
        HIPCHK(hipMalloc(&ds.scratch, plan_bytes));
        ds.scratch_bytes = plan_bytes;
    }
    P.base = static_cast<char*>(ds.scratch);
    return 0;
}

static int build_tree(DeviceScene& ds, hipStream_t stream, const TreePlan& P, uint n, TriRecord* out_tris, Bvh4Node* out_nodes) {
    char* base = P.base;
    size_t sort_bytes = P.sort_bytes, scan_bytes = P.scan_bytes;
    const size_t o_cbounds = P.o_cbounds, o_unsorted = P.o_unsorted, o_keys = P.o_keys, o_keys_sorted = P.o_keys_sorted, o_vals = P.o_vals,
                 o_vals_sorted = P.o_vals_sorted, o_leaf_box = P.o_leaf_box, o_sort = P.o_sort, o_children = P.o_children, o_sizes = P.o_sizes,
                 o_parent = P.o_parent, o_parent_leaf = P.o_parent_leaf, o_node_box = P.o_node_box, o_arrive = P.o_arrive, o_cref0 = P.o_cref0,
                 o_cref1 = P.o_cref1, o_cbox0 = P.o_cbox0, o_cbox1 = P.o_cbox1, o_nn = P.o_nn, o_valid = P.o_valid, o_pos = P.o_pos, o_scan = P.o_scan,
                 o_new_id = P.o_new_id, o_nodes2 = P.o_nodes2, o_uparent = P.o_uparent, o_moves = P.o_moves, o_lock = P.o_lock, o_optstat = P.o_optstat,
                 o_ccost = P.o_ccost, o_cdec = P.o_cdec;
    (void)o_cbounds;
    uint* cbounds = P.cbounds();
    const uint n_tri = n;
    const bool optimise = ds.optimise_rounds > 0 && !ds.fast_build && n_tri > 2;
    const bool dp_collapse = ds.collapse_by_cost && !ds.fast_build && n_tri > 2;
    if (n_tri > 0) {
        TriRecord* unsorted = reinterpret_cast<TriRecord*>(base + o_unsorted);
        unsigned long long *keys = reinterpret_cast<unsigned long long*>(base + o_keys), *keys_sorted = reinterpret_cast<unsigned long long*>(base + o_keys_sorted);
        uint *vals = reinterpret_cast<uint*>(base + o_vals), *vals_sorted = reinterpret_cast<uint*>(base + o_vals_sorted);
        float *leaf_box = reinterpret_cast<float*>(base + o_leaf_box), *node_box = reinterpret_cast<float*>(base + o_node_box);
        int2* children = reinterpret_cast<int2*>(base + o_children);
        uint* ranges = reinterpret_cast<uint*>(base + o_sizes);   // subtree sizes (leaves per internal node)
        int *parent_internal = reinterpret_cast<int*>(base + o_parent), *parent_leaf = reinterpret_cast<int*>(base + o_parent_leaf);
        uint* arrive = reinterpret_cast<uint*>(base + o_arrive);
        BvhNode* nodes2 = reinterpret_cast<BvhNode*>(base + o_nodes2);   // binary nodes: only the collapse input
        const uint blocks = (n + BT - 1) / BT;
        hipLaunchKernelGGL(k_morton, dim3(blocks), dim3(BT), 0, stream, n, unsorted, cbounds, keys, vals);
        HIPCHK(rocprim::radix_sort_pairs(base + o_sort, sort_bytes, keys, keys_sorted, vals, vals_sorted, n, 0, 64, stream));
        hipLaunchKernelGGL(k_gather_leaves, dim3(blocks), dim3(BT), 0, stream, n, unsorted, vals_sorted, out_tris, leaf_box);
        const size_t n_all = (size_t)n + (n > 1 ? n - 1 : 0);
        if (n > 1) {
            const uint iblocks = (n - 1 + BT - 1) / BT;
            if (ds.builder == 0) {
                // Karras 2012 LBVH + atomic bottom-up refit
                HIPCHK(hipMemsetAsync(arrive, 0, (size_t)(n - 1) * 4, stream));
                hipLaunchKernelGGL(k_hierarchy, dim3(iblocks), dim3(BT), 0, stream, (int)n, keys_sorted, children, ranges, parent_internal, parent_leaf);
                hipLaunchKernelGGL(k_refit, dim3(blocks), dim3(BT), 0, stream, (int)n, children, parent_internal, parent_leaf, leaf_box,
                                   node_box, arrive, nodes2);
            } else {
                // PLOC over the Morton order
                int* cref[2] = {reinterpret_cast<int*>(base + o_cref0), reinterpret_cast<int*>(base + o_cref1)};
                float* cbox[2] = {reinterpret_cast<float*>(base + o_cbox0), reinterpret_cast<float*>(base + o_cbox1)};
                uint *nn = reinterpret_cast<uint*>(base + o_nn), *valid = reinterpret_cast<uint*>(base + o_valid), *pos = reinterpret_cast<uint*>(base + o_pos);
                uint *alloc = cbounds + 6, *c_dev = cbounds + 8;   // count of round r in c_dev[r & 1]; k_ploc_compact writes the other one
                HIPCHK(hipMemsetAsync(parent_internal, 0xFF, (size_t)(n - 1) * 4, stream));   // root keeps -1
                hipLaunchKernelGGL(k_ploc_init, dim3(blocks), dim3(BT), 0, stream, n, cref[0]);
                HIPCHK(hipMemcpyAsync(cbox[0], leaf_box, (size_t)n * 24, hipMemcpyDeviceToDevice, stream));
                HIPCHK(hipMemcpyAsync(c_dev, &n, 4, hipMemcpyHostToDevice, stream));
                uint c = n;   // last cluster count the host has seen (upper bound of the live count)
                int rounds = 0;
                const bool tail = !getenv("TRHIP_PLOC_NO_TAIL");
                while (c > 1) {
                    if (tail && c <= PLOC_TAIL) {   // the rest in one workgroup; its round count stays on the device (cbounds[10])
                        hipLaunchKernelGGL(k_ploc_tail, dim3(1), dim3(PLOC_TAIL), 0, stream, c_dev + (rounds & 1), n, (uint)ds.ploc_radius, cref[0], cbox[0], alloc,
                                           children, node_box, ranges, parent_internal, cbounds + 10);
                        break;
                    }
                    // rounds between host checks: few while the grids are large (an over-sized grid costs), many once they are small
                    const int batch = c > (1u << 16) ? 2 : (c > 4096 ? 4 : 8);
                    const uint cb = (c + BT - 1) / BT;
                    for (int r = 0; r < batch; ++r) {
                        const uint* c_cur = c_dev + ((rounds + r) & 1);
                        hipLaunchKernelGGL(k_ploc_nn, dim3(cb), dim3(BT), 0, stream, c_cur, (uint)ds.ploc_radius, cbox[0], nn);
                        hipLaunchKernelGGL(k_ploc_merge, dim3(cb), dim3(BT), 0, stream, c_cur, n, cref[0], cbox[0], nn, valid, cref[1], cbox[1], alloc, children,
                                           node_box, ranges, parent_internal);
                        HIPCHK(rocprim::exclusive_scan(base + o_scan, scan_bytes, valid, pos, 0u, cb * BT, rocprim::plus<uint>(), stream));
                        hipLaunchKernelGGL(k_ploc_compact, dim3(cb), dim3(BT), 0, stream, c_cur, c_dev + ((rounds + r + 1) & 1), valid, pos, cref[1], cbox[1], cref[0], cbox[0]);
                    }
                    rounds += batch;
                    uint c_new = 0;
                    HIPCHK(hipMemcpyAsync(&c_new, c_dev + (rounds & 1), 4, hipMemcpyDeviceToHost, stream));
                    HIPCHK(hipStreamSynchronize(stream));
                    if (c_new >= c || rounds > 4096) return set_error("PLOC: clustering did not converge");
                    c = c_new;
                }
                ds.build_rounds = (uint)rounds;
            }
            if (optimise) {
                // static geometry, "prefer fast trace": reinsertion rounds on the binary tree (bvh_optimize.h)
                OptTree t{(uint)(n - 1), n, children, node_box, leaf_box, reinterpret_cast<int*>(base + o_uparent)};
                OptMove* moves = reinterpret_cast<OptMove*>(base + o_moves);
                unsigned long long* lock = reinterpret_cast<unsigned long long*>(base + o_lock);
                double* cost = reinterpret_cast<double*>(base + o_optstat);
                uint* applied = reinterpret_cast<uint*>(base + o_optstat + 16);
                const uint ablocks = (uint)((n_all + BT - 1) / BT);
                const bool debug = getenv("TRHIP_DEBUG") != nullptr;
                auto report = [&](int round) -> int {
                    if (!debug) return 0;
                    double h[3] = {0, 0, 0};
                    HIPCHK(hipMemsetAsync(cost, 0, 8, stream));
                    hipLaunchKernelGGL(k_opt_cost, dim3(iblocks), dim3(BT), 0, stream, t, cost);
                    HIPCHK(hipMemcpyAsync(h, cost, 24, hipMemcpyDeviceToHost, stream));
                    HIPCHK(hipStreamSynchronize(stream));
                    uint moved[2]; memcpy(moved, &h[2], 8);
                    fprintf(stderr, "[trhip] tree optimisation round %d: inner area sum %.6g, %u of %u moves applied\n", round, h[0], round ? moved[0] : 0u, round ? moved[1] : 0u);
                    if (round) {   // every box against its children, every leaf count, every parent link
                        uint bad = 0;
                        HIPCHK(hipMemsetAsync(applied, 0, 4, stream));
                        hipLaunchKernelGGL(k_opt_check, dim3(iblocks), dim3(BT), 0, stream, t, ranges, applied);
                        HIPCHK(hipMemcpyAsync(&bad, applied, 4, hipMemcpyDeviceToHost, stream));
                        HIPCHK(hipStreamSynchronize(stream));
                        if (bad) return set_error("tree optimisation: " + std::to_string(bad) + " inconsistent nodes after round " + std::to_string(round));
                    }
                    return 0;
                };
                hipLaunchKernelGGL(k_opt_parents, dim3(iblocks), dim3(BT), 0, stream, t);
                if (int rc = report(0)) return rc;
                for (int round = 0; round < ds.optimise_rounds; ++round) {
                    HIPCHK(hipMemsetAsync(lock, 0, n_all * 8, stream));
                    HIPCHK(hipMemsetAsync(applied, 0, 8, stream));
                    HIPCHK(hipMemsetAsync(arrive, 0, (size_t)(n - 1) * 4, stream));
                    hipLaunchKernelGGL(k_opt_search, dim3(ablocks), dim3(BT), 0, stream, t, moves, (uint)round % (uint)ds.optimise_modulus, (uint)ds.optimise_modulus);
                    hipLaunchKernelGGL(k_opt_lock, dim3(ablocks), dim3(BT), 0, stream, t, moves, lock, debug ? applied + 1 : nullptr);
                    hipLaunchKernelGGL(k_opt_verify, dim3(ablocks), dim3(BT), 0, stream, t, moves, lock);
                    hipLaunchKernelGGL(k_opt_apply, dim3(ablocks), dim3(BT), 0, stream, t, moves, applied);
                    hipLaunchKernelGGL(k_opt_refit, dim3(blocks), dim3(BT), 0, stream, t, arrive, ranges);
                    if (int rc = report(round + 1)) return rc;
                }
                parent_internal = t.parent;     // the first n - 1 entries are the inner nodes' parents
            }
            {
                int* new_id = reinterpret_cast<int*>(base + o_new_id);
                if (ds.dfs_layout) hipLaunchKernelGGL(k_dfs_order, dim3(iblocks), dim3(BT), 0, stream, n - 1, children, ranges, parent_internal, new_id);
                else hipLaunchKernelGGL(k_identity, dim3(iblocks), dim3(BT), 0, stream, n - 1, new_id);
                const uint8_t* dec = nullptr;
                if (dp_collapse) {
                    OptTree t{(uint)(n - 1), n, children, node_box, leaf_box, reinterpret_cast<int*>(base + o_uparent)};
                    if (!optimise) hipLaunchKernelGGL(k_opt_parents, dim3(iblocks), dim3(BT), 0, stream, t);
                    HIPCHK(hipMemsetAsync(arrive, 0, (size_t)(n - 1) * 4, stream));
                    hipLaunchKernelGGL(k_collapse_cost, dim3(blocks), dim3(BT), 0, stream, t, arrive, reinterpret_cast<float*>(base + o_ccost), reinterpret_cast<uint8_t*>(base + o_cdec));
                    dec = reinterpret_cast<const uint8_t*>(base + o_cdec);
                }
                hipLaunchKernelGGL(k_collapse4, dim3(iblocks), dim3(BT), 0, stream, n - 1, children, node_box, leaf_box, new_id, dec, out_nodes);
            }
        }
        HIPCHK(hipGetLastError());
    }
    return 0;
}

static int build_two_level(DeviceScene& ds, hipStream_t stream, trhip_accel_info* info);
static int refit_two_level(DeviceScene& ds, hipStream_t stream, trhip_accel_info* info);

int build_accel(DeviceScene& ds, hipStream_t stream, trhip_accel_info* info) {
    if (ds.accel_strategy != TRHIP_AS_ALL_MERGED) return build_two_level(ds, stream, info);
    const uint n_scene = ds.tri_count;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    HIPCHK(hipEventRecord(e0, stream));
    ds.accel_built = false;
    ds.levels_valid = false;   // a new tree: the refit level lists are rebuilt on demand
    SceneView sv = ds.view();
    sv.tri_count = n_scene;
    // Temporaries come out of one scratch arena that survives the call, and the outputs keep their allocation while the
    // triangle count does not change: a rebuild (dynamic scenes) performs no allocation at all.
    // n_tri = triangles = leaves; n_cap = what everything is sized for
    const uint n_tri = n_scene;
    const uint n_cap = n_tri;
    uint n = n_tri;
    const size_t n1 = n_cap > 1 ? n_cap - 1 : 0;     // inner nodes the buffers hold
    if (ds.two_level) ds.free_accel();                // the outputs of a two-level build
    TreePlan P;
    if (int rc = plan_tree(ds, stream, n_cap, P)) return rc;
    uint* cbounds = P.cbounds();
    {
        const uint init[32] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(cbounds, init, sizeof(init), hipMemcpyHostToDevice, stream));
    }
    if (ds.accel_capacity != n_cap) {   // outputs
        ds.free_accel();
        if (n_cap > 0) HIPCHK(hipMalloc(&ds.tris, (size_t)n_cap * sizeof(TriRecord) + sizeof(EmitterSet)));      // the emitter set sits behind the records
        if (n1 > 0) {
            // traversal addresses a node's planes with 32-bit byte offsets (node << 7 | plane)
            if ((uint64_t)n1 * sizeof(Bvh4Node) > 0xFFFFFFFFull) return set_error("trhip_scene_build_accel: more than 2^25 nodes");
            HIPCHK(hipMalloc(&ds.nodes4, n1 * sizeof(Bvh4Node)));
        }
        ds.accel_capacity = n_cap;
    }
    if (n_tri > 0) {
        TriRecord* unsorted = P.unsorted();
        const uint tblocks = (n_tri + BT - 1) / BT;
        hipLaunchKernelGGL(k_pretransform, dim3(tblocks < 1024u ? tblocks : 1024u), dim3(BT), 0, stream, sv, ds.tri_prefix, ds.non_opaque, ds.alpha_base, ds.alpha_tris, unsorted, cbounds);
    }
    if (int rc = build_tree(ds, stream, P, n, ds.tris, ds.nodes4)) return rc;
    ds.leaf_count = n;
    ds.node_count = n > 1 ? n - 1 : 0;
    ds.accel_tri_count = n_tri;
    ds.accel_built = true;
    // tri lights
    ds.tri_light_count = 0;
    if (ds.gather_emissive_triangles && ds.host_tri_light_count > 0) {
        if (!ds.tri_lights) HIPCHK(hipMalloc(&ds.tri_lights, (size_t)ds.host_tri_light_count * sizeof(TriLight)));
        HIPCHK(hipMemsetAsync(ds.tri_lights, 0, (size_t)ds.host_tri_light_count * sizeof(TriLight), stream));
        ds.tri_light_count = ds.host_tri_light_count;
        SceneView sv2 = ds.view();
        hipLaunchKernelGGL(k_extract_tri_lights, dim3((n_tri + BT - 1) / BT), dim3(BT), 0, stream, sv2, ds.tri_prefix, ds.tri_lights);
        HIPCHK(hipGetLastError());
    }
    if (int rc = gather_emitters(ds, stream)) return rc;
    HIPCHK(hipEventRecord(e1, stream));
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    uint hb[6];
    HIPCHK(hipMemcpy(hb, cbounds, sizeof(hb), hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k) { ds.bounds_lo[k] = float_unflip(hb[k]); ds.bounds_hi[k] = float_unflip(hb[3 + k]); }
    ds.layout = {};
    ds.layout.strategy = TRHIP_AS_ALL_MERGED; ds.layout.blas_count = 1; ds.layout.blas_updated = 1;
    ds.layout.node_bytes = (uint64_t)ds.node_count * sizeof(Bvh4Node); ds.layout.record_bytes = (uint64_t)n * sizeof(TriRecord);
    ds.layout.blas_ms = ms;
    if (info) {
        info->triangle_count = n_tri;
        info->leaf_count = n;
        info->node_count = ds.node_count;
        info->node_bytes = 112u;
        info->tri_light_count = ds.tri_light_count;
        info->build_ms = ms;
        for (int k = 0; k < 3; ++k) { info->bounds_min[k] = float_unflip(hb[k]); info->bounds_max[k] = float_unflip(hb[3 + k]); }
    }
    return 0;
}

// =====================================================================================================================
// Two-level structure (trhip_scene_set_accel_strategy): one BLAS per group of instances, built by build_tree into
// the shared node and record arrays behind the TLAS slots, and a TLAS built by the same pipeline over the instances' world boxes (a box
// record is a TriRecord with v0 = lo, v1 = hi, v2 = lo: every stage takes a record's box as min / max of its three vertices).
namespace {

// records of one BLAS.  `list` = the instances whose triangles it holds (prefix sums of their triangle counts in `prefix`); world: the
// merged static BLAS, records as k_pretransform writes them; else one instance of the shared span, object-space positions as uploaded.
__global__ __launch_bounds__(BT) void k_group_records(SceneView sv, const uint* list, const uint* prefix, uint n_list, uint n, int world,
                                                      const uint8_t* non_opaque, const uint* alpha_base, AlphaTri* alpha_tris, TriRecord* out) {
    const uint gid = blockIdx.x * BT + threadIdx.x;
    if (gid >= n) return;
    uint slot, prim;
    locate_triangle(prefix, n_list, gid, slot, prim);
    const uint inst = list[slot];
    const MeshSpan sp = sv.obj_spans[inst];
    const uint* ix = sv.indices + sp.index_offset + 3u * prim;
    const Vertex* vb = sv.obj_vertices + sp.vertex_offset;
    f3 p0 = vb[ix[0]].pos, p1 = vb[ix[1]].pos, p2 = vb[ix[2]].pos;
    TriRecord t;
    if (world) {
        const m4 model = sv.instances[inst].model;
        p0 = transform_point(model, p0); p1 = transform_point(model, p1); p2 = transform_point(model, p2);
        t.inst_flags = inst | (non_opaque[inst] ? 0x80000000u : 0u);
        t.alpha = non_opaque[inst] ? alpha_word(sv.instances[inst].mat, alpha_base[inst] + prim, alpha_tris, vb[ix[0]].uv, vb[ix[1]].uv, vb[ix[2]].uv) : 0u;
    } else {
        t.inst_flags = inst;     // the instance the refit reads the span from; the traversal takes the words from the TLAS leaf
        t.alpha = 0u;
    }
    t.prim = prim;
    t.v0[0] = p0.x; t.v0[1] = p0.y; t.v0[2] = p0.z;
    t.v1[0] = p1.x; t.v1[1] = p1.y; t.v1[2] = p1.z;
    t.v2[0] = p2.x; t.v2[1] = p2.y; t.v2[2] = p2.z;
    out[gid] = t;
}

// the centroid and box bounds k_pretransform accumulates, for records that are already written
__global__ __launch_bounds__(BT) void k_record_bounds(uint n, const TriRecord* recs, uint* cbounds) {
    float cmin[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float cmax[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    float smin[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()};
    float smax[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    for (uint i = blockIdx.x * BT + threadIdx.x; i < n; i += gridDim.x * BT) {
        const TriRecord t = recs[i];
        for (int k = 0; k < 3; ++k) {
            const float lo = fminf(fminf(t.v0[k], t.v1[k]), t.v2[k]), hi = fmaxf(fmaxf(t.v0[k], t.v1[k]), t.v2[k]);
            const float c = (lo + hi) * 0.5f;
            cmin[k] = fminf(cmin[k], c); cmax[k] = fmaxf(cmax[k], c); smin[k] = fminf(smin[k], lo); smax[k] = fmaxf(smax[k], hi);
        }
    }
    __shared__ float s_red[BT / 64][12];
    for (int k = 0; k < 3; ++k) {
        float mn = cmin[k], mx = cmax[k], sn = smin[k], sx = smax[k];
        for (int off = 32; off > 0; off >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, off)); mx = fmaxf(mx, __shfl_xor(mx, off));
            sn = fminf(sn, __shfl_xor(sn, off)); sx = fmaxf(sx, __shfl_xor(sx, off));
        }
        if ((threadIdx.x & 63) == 0) { float* w = s_red[threadIdx.x >> 6]; w[k] = mn; w[3 + k] = mx; w[6 + k] = sn; w[9 + k] = sx; }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int k = (int)threadIdx.x;
        float mn = s_red[0][k], mx = s_red[0][3 + k], sn = s_red[0][6 + k], sx = s_red[0][9 + k];
        for (int w = 1; w < BT / 64; ++w) { mn = fminf(mn, s_red[w][k]); mx = fmaxf(mx, s_red[w][3 + k]); sn = fminf(sn, s_red[w][6 + k]); sx = fmaxf(sx, s_red[w][9 + k]); }
        if (mn <= mx) {
            atomicMin(&cbounds[k], float_flip(mn)); atomicMax(&cbounds[3 + k], float_flip(mx));
            atomicMin(&cbounds[16 + k], float_flip(sn)); atomicMax(&cbounds[19 + k], float_flip(sx));
        }
    }
}

// the AlphaTri records of every non-opaque instance (in a shared BLAS the record words do not carry them)
__global__ __launch_bounds__(BT) void k_alpha_records(SceneView sv, const uint* tri_prefix, const uint8_t* non_opaque, const uint* alpha_base, AlphaTri* alpha_tris) {
    const uint gid = blockIdx.x * BT + threadIdx.x;
    if (gid >= sv.tri_count) return;
    uint inst, prim;
    locate_triangle(tri_prefix, sv.instance_count, gid, inst, prim);
    if (!non_opaque[inst]) return;
    const MeshSpan sp = sv.obj_spans[inst];
    const uint* ix = sv.indices + sp.index_offset + 3u * prim;
    const Vertex* vb = sv.obj_vertices + sp.vertex_offset;
    (void)alpha_word(sv.instances[inst].mat, alpha_base[inst] + prim, alpha_tris, vb[ix[0]].uv, vb[ix[1]].uv, vb[ix[2]].uv);
}

// ... of the triangles of the instances in `list` (prefix sums of their triangle counts in `prefix`): a refit's stale records only
__global__ __launch_bounds__(BT) void k_alpha_list(SceneView sv, const uint* list, const uint* prefix, uint n_list, uint n, const uint* alpha_base,
                                                   AlphaTri* alpha_tris) {
    const uint gid = blockIdx.x * BT + threadIdx.x;
    if (gid >= n) return;
    uint slot, prim;
    locate_triangle(prefix, n_list, gid, slot, prim);
    const uint inst = list[slot];
    const MeshSpan sp = sv.obj_spans[inst];
    const uint* ix = sv.indices + sp.index_offset + 3u * prim;
    const Vertex* vb = sv.obj_vertices + sp.vertex_offset;
    (void)alpha_word(sv.instances[inst].mat, alpha_base[inst] + prim, alpha_tris, vb[ix[0]].uv, vb[ix[1]].uv, vb[ix[2]].uv);
}

// a BLAS built at node 0 / record 0 moved to its place in the shared arrays
__global__ __launch_bounds__(BT) void k_rebase(Bvh4Node* nodes, uint count, int node_off, int tri_off) {
    const uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= count) return;
    for (int c = 0; c < 4; ++c) {
        const int ch = nodes[i].child[c];
        if (ch == 0x7FFFFFFF) continue;
        nodes[i].child[c] = ch >= 0 ? ch + node_off : ~(~ch + tri_off);
    }
}

// the box of each BLAS root reference (a node: the union of its child boxes; a record: its triangle)
__global__ __launch_bounds__(BT) void k_root_boxes(const Bvh4Node* nodes, const TriRecord* tris, const int* roots, uint n, float* out) {
    const uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    float lo[3] = {__builtin_huge_valf(), __builtin_huge_valf(), __builtin_huge_valf()}, hi[3] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf()};
    const int r = roots[i];
    if (r >= 0) {
        const Bvh4Node& nd = nodes[r];
        for (int c = 0; c < 4; ++c) {
            if (nd.child[c] == 0x7FFFFFFF) continue;
            lo[0] = fminf(lo[0], nd.lox[c]); lo[1] = fminf(lo[1], nd.loy[c]); lo[2] = fminf(lo[2], nd.loz[c]);
            hi[0] = fmaxf(hi[0], nd.hix[c]); hi[1] = fmaxf(hi[1], nd.hiy[c]); hi[2] = fmaxf(hi[2], nd.hiz[c]);
        }
    } else {
        const TriRecord& t = tris[~r];
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(fminf(t.v0[k], t.v1[k]), t.v2[k]); hi[k] = fmaxf(fmaxf(t.v0[k], t.v1[k]), t.v2[k]); }
    }
    for (int k = 0; k < 3; ++k) { out[6 * i + k] = lo[k]; out[6 * i + 3 + k] = hi[k]; }
}

// instance records in TLAS leaf order: a sorted box record's `prim` is the leaf's place in the build input
__global__ __launch_bounds__(BT) void k_tlas_leaves(uint n, const TriRecord* sorted, const TlasLeaf* src, TlasLeaf* out) {
    const uint i = blockIdx.x * BT + threadIdx.x;
    if (i < n) out[i] = src[sorted[i].prim];
}

// object-space records of a shared BLAS after skinning (k_retransform without the transform)
__global__ __launch_bounds__(BT) void k_retransform_obj(SceneView sv, uint n, TriRecord* tris) {
    const uint i = blockIdx.x * BT + threadIdx.x;
    if (i >= n) return;
    TriRecord t = tris[i];
    const MeshSpan sp = sv.obj_spans[t.inst_flags & 0x7FFFFFFFu];
    const uint* ix = sv.indices + sp.index_offset + 3u * t.prim;
    const Vertex* vb = sv.obj_vertices + sp.vertex_offset;
    const f3 p0 = vb[ix[0]].pos, p1 = vb[ix[1]].pos, p2 = vb[ix[2]].pos;
    t.v0[0] = p0.x; t.v0[1] = p0.y; t.v0[2] = p0.z;
    t.v1[0] = p1.x; t.v1[1] = p1.y; t.v1[2] = p1.z;
    t.v2[0] = p2.x; t.v2[1] = p2.y; t.v2[2] = p2.z;
    tris[i] = t;
}

const uint kCboundsInit[32] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};

bool is_identity(const m4& m) {
    const float* a = &m.c[0].x;
    for (int k = 0; k < 16; ++k) if (a[k] != ((k % 5 == 0) ? 1.0f : 0.0f)) return false;
    return true;
}

// world -> object rows of an affine model matrix (column-major m4; the bottom row is taken as 0 0 0 1), inverted in double.  An exact
// identity gives an exact identity, and TR_TLAS_IDENTITY then skips the transform altogether.
void inverse_rows(const m4& m, float xf[12]) {
    double a[3][3], t[3];
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) a[r][c] = (double)(&m.c[c].x)[r];
        t[r] = (double)(&m.c[3].x)[r];
    }
    double inv[3][3];
    inv[0][0] = a[1][1] * a[2][2] - a[1][2] * a[2][1]; inv[0][1] = a[0][2] * a[2][1] - a[0][1] * a[2][2]; inv[0][2] = a[0][1] * a[1][2] - a[0][2] * a[1][1];
    inv[1][0] = a[1][2] * a[2][0] - a[1][0] * a[2][2]; inv[1][1] = a[0][0] * a[2][2] - a[0][2] * a[2][0]; inv[1][2] = a[0][2] * a[1][0] - a[0][0] * a[1][2];
    inv[2][0] = a[1][0] * a[2][1] - a[1][1] * a[2][0]; inv[2][1] = a[0][1] * a[2][0] - a[0][0] * a[2][1]; inv[2][2] = a[0][0] * a[1][1] - a[0][1] * a[1][0];
    const double det = a[0][0] * inv[0][0] + a[0][1] * inv[1][0] + a[0][2] * inv[2][0];
    for (int r = 0; r < 3; ++r) {
        double o = 0.0;
        for (int c = 0; c < 3; ++c) { const double v = inv[r][c] / det; xf[4 * r + c] = (float)v; o -= v * t[c]; }
        xf[4 * r + 3] = (float)o;
    }
}

int ensure_aux(DeviceScene& ds, size_t bytes) {
    if (bytes <= ds.tl_aux_bytes) return 0;
    if (ds.tl_aux) (void)hipFree(ds.tl_aux);
    ds.tl_aux = nullptr; ds.tl_aux_bytes = 0;
    HIPCHK(hipMalloc(&ds.tl_aux, bytes));
    ds.tl_aux_bytes = bytes;
    return 0;
}

// The TLAS over the current instance transforms: BLAS root boxes -> world boxes (on the host, in double, rounded outwards) -> build_tree
// into node slots 0 .. L - 2 -> instance records in leaf order.
int build_tlas(DeviceScene& ds, hipStream_t stream, const TreePlan& P) {
    const uint nb = (uint)ds.blases.size(), L = ds.tlas_leaf_count;
    const size_t o_boxes = ((size_t)nb * 4 + 255) & ~(size_t)255, o_sorted = o_boxes + (((size_t)nb * 24 + 255) & ~(size_t)255);
    if (int rc = ensure_aux(ds, o_sorted + (size_t)L * sizeof(TriRecord))) return rc;
    char* aux = static_cast<char*>(ds.tl_aux);
    std::vector<int> roots(nb);
    for (uint b = 0; b < nb; ++b) roots[b] = ds.blases[b].root;
    std::vector<float> boxes((size_t)nb * 6);
    if (nb) {
        HIPCHK(hipMemcpyAsync(aux, roots.data(), (size_t)nb * 4, hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_root_boxes, dim3((nb + BT - 1) / BT), dim3(BT), 0, stream, ds.nodes4, ds.tris, reinterpret_cast<const int*>(aux), nb,
                           reinterpret_cast<float*>(aux + o_boxes));
        HIPCHK(hipMemcpyAsync(boxes.data(), aux + o_boxes, (size_t)nb * 24, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
    }
    std::vector<TlasLeaf> leaves(L);
    std::vector<TriRecord> recs(L);
    for (uint j = 0; j < L; ++j) {
        const uint inst = ds.tlas_src[j];
        const int b = inst == 0xFFFFFFFFu ? 0 : ds.inst_blas[inst];
        const float* bx = &boxes[(size_t)b * 6];
        TlasLeaf& lf = leaves[j];
        memset(&lf, 0, sizeof(lf));
        lf.blas_root = ds.blases[b].root;
        float lo[3] = {bx[0], bx[1], bx[2]}, hi[3] = {bx[3], bx[4], bx[5]};
        const bool ident = inst == 0xFFFFFFFFu || is_identity(ds.host_instances[inst].model);
        if (ident) {
            lf.xf[0] = lf.xf[5] = lf.xf[10] = 1.0f;
            lf.flags = TR_TLAS_IDENTITY;
        } else {
            const m4& m = ds.host_instances[inst].model;
            inverse_rows(m, lf.xf);
            double wlo[3] = {1e300, 1e300, 1e300}, whi[3] = {-1e300, -1e300, -1e300};
            for (int c = 0; c < 8; ++c) {
                const double p[3] = {(c & 1) ? bx[3] : bx[0], (c & 2) ? bx[4] : bx[1], (c & 4) ? bx[5] : bx[2]};
                for (int r = 0; r < 3; ++r) {
                    double w = (double)(&m.c[3].x)[r];
                    for (int k = 0; k < 3; ++k) w += (double)(&m.c[k].x)[r] * p[k];
                    wlo[r] = std::min(wlo[r], w); whi[r] = std::max(whi[r], w);
                }
            }
            // outwards by a relative 2^-16 of the box's size and place: covers the rounding of the object-space ray (a few ulp of the
            // coordinates involved), so that no hit of the BLAS lies outside the box the world ray is tested against
            for (int r = 0; r < 3; ++r) {
                const double pad = (std::fabs(wlo[r]) + std::fabs(whi[r]) + (whi[r] - wlo[r])) * (1.0 / 65536.0);
                lo[r] = std::nextafter((float)(wlo[r] - pad), -INFINITY); hi[r] = std::nextafter((float)(whi[r] + pad), INFINITY);
            }
        }
        if (inst == 0xFFFFFFFFu) { lf.inst_word = TR_INST_FROM_RECORD; lf.alpha_base = 0; }
        else {
            lf.inst_word = inst | (ds.host_non_opaque[inst] ? 0x80000000u : 0u);
            lf.alpha_base = ds.host_non_opaque[inst] ? ds.host_alpha_base[inst] : 0u;
        }
        TriRecord& t = recs[j];
        memset(&t, 0, sizeof(t));
        for (int k = 0; k < 3; ++k) { t.v0[k] = lo[k]; t.v1[k] = hi[k]; t.v2[k] = lo[k]; }
        t.prim = j;
        for (int k = 0; k < 3; ++k) {    // trhip_accel_info bounds of a two-level structure: the union of the instances' world boxes
            ds.bounds_lo[k] = j == 0 ? lo[k] : std::min(ds.bounds_lo[k], lo[k]);
            ds.bounds_hi[k] = j == 0 ? hi[k] : std::max(ds.bounds_hi[k], hi[k]);
        }
    }
    if (L == 0) { for (int k = 0; k < 3; ++k) ds.bounds_lo[k] = ds.bounds_hi[k] = 0.0f; return 0; }
    if (L == 1) {   // the root is a node of one child, so that every two-level traversal starts at node 0
        Bvh4Node root;
        for (int c = 0; c < 4; ++c) {
            root.lox[c] = root.loy[c] = root.loz[c] = INFINITY; root.hix[c] = root.hiy[c] = root.hiz[c] = -INFINITY;
            root.child[c] = 0x7FFFFFFF; root.pad[c] = 0;
        }
        root.lox[0] = recs[0].v0[0]; root.loy[0] = recs[0].v0[1]; root.loz[0] = recs[0].v0[2];
        root.hix[0] = recs[0].v1[0]; root.hiy[0] = recs[0].v1[1]; root.hiz[0] = recs[0].v1[2];
        root.child[0] = ~0;
        HIPCHK(hipMemcpyAsync(ds.nodes4, &root, sizeof(root), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(ds.tlas, leaves.data(), sizeof(TlasLeaf), hipMemcpyHostToDevice, stream));
        HIPCHK(hipStreamSynchronize(stream));      // `root` and `leaves` live on this stack
        return 0;
    }
    HIPCHK(hipMemcpyAsync(ds.tlas_src_leaves, leaves.data(), (size_t)L * sizeof(TlasLeaf), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(P.unsorted(), recs.data(), (size_t)L * sizeof(TriRecord), hipMemcpyHostToDevice, stream));
    HIPCHK(hipMemcpyAsync(P.cbounds(), kCboundsInit, sizeof(kCboundsInit), hipMemcpyHostToDevice, stream));
    HIPCHK(hipStreamSynchronize(stream));      // `leaves` and `recs` live in this function
    const uint blocks = (L + BT - 1) / BT;
    hipLaunchKernelGGL(k_record_bounds, dim3(blocks < 1024u ? blocks : 1024u), dim3(BT), 0, stream, L, P.unsorted(), P.cbounds());
    TriRecord* sorted = reinterpret_cast<TriRecord*>(aux + o_sorted);
    if (int rc = build_tree(ds, stream, P, L, sorted, ds.nodes4)) return rc;
    hipLaunchKernelGGL(k_tlas_leaves, dim3(blocks), dim3(BT), 0, stream, L, sorted, ds.tlas_src_leaves, ds.tlas);
    HIPCHK(hipGetLastError());
    return 0;
}

int extract_tri_lights(DeviceScene& ds, hipStream_t stream) {
    ds.tri_light_count = 0;
    if (ds.gather_emissive_triangles && ds.host_tri_light_count > 0) {
        if (!ds.tri_lights) HIPCHK(hipMalloc(&ds.tri_lights, (size_t)ds.host_tri_light_count * sizeof(TriLight)));
        HIPCHK(hipMemsetAsync(ds.tri_lights, 0, (size_t)ds.host_tri_light_count * sizeof(TriLight), stream));
        ds.tri_light_count = ds.host_tri_light_count;
        SceneView sv2 = ds.view();
        hipLaunchKernelGGL(k_extract_tri_lights, dim3((ds.tri_count + BT - 1) / BT), dim3(BT), 0, stream, sv2, ds.tri_prefix, ds.tri_lights);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

void fill_info(const DeviceScene& ds, trhip_accel_info* info, float ms) {
    if (!info) return;
    memset(info, 0, sizeof(*info));
    info->triangle_count = ds.tri_count; info->leaf_count = ds.leaf_count; info->node_count = ds.node_count; info->node_bytes = 112u;
    info->tri_light_count = ds.tri_light_count; info->build_ms = ms;
    for (int k = 0; k < 3; ++k) { info->bounds_min[k] = ds.bounds_lo[k]; info->bounds_max[k] = ds.bounds_hi[k]; }
}

struct Timer {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Timer() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
};

}  // namespace

void mark_skinned(DeviceScene& ds, uint instance) {
    if (!ds.two_level || instance >= ds.inst_blas.size() || ds.inst_blas[instance] < 0) return;
    if (ds.host_non_opaque[instance]) ds.alpha_dirty[instance] = 1;
    const int b = ds.inst_blas[instance];
    if (ds.blases[b].world) ds.static_dirty = true;
    else ds.blas_dirty[b] = 1;
}

static int build_two_level(DeviceScene& ds, hipStream_t stream, trhip_accel_info* info) {
    Timer T;
    for (hipEvent_t& x : T.e) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipEventRecord(T.e[0], stream));
    ds.accel_built = false;
    ds.levels_valid = false;
    if (!ds.two_level) ds.free_accel();      // the outputs of an all-merged build
    const uint NI = ds.instance_count;
    const bool merge_static = ds.accel_strategy == TRHIP_AS_STATIC_MERGED_DYNAMIC_PER_MESH;
    // grouping: a span key per instance; an instance is dynamic when marked, skinned, or on the span of a skinned instance
    auto key = [&](uint i) { const MeshSpan& s = ds.host_spans[i]; return std::make_tuple(s.vertex_offset, s.vertex_count, s.index_offset, s.triangle_count); };
    std::vector<std::tuple<uint, uint, uint, uint>> skinned_keys;
    for (uint i = 0; i < NI && i < ds.skin_slots.size(); ++i) if (ds.skin_slots[i].source) skinned_keys.push_back(key(i));
    for (uint i = 0; i < NI; ++i) if (ds.has_morph(i)) skinned_keys.push_back(key(i));      // a morphed mesh deforms like a skinned one
    std::vector<uint8_t> dyn(NI, 0);
    for (uint i = 0; i < NI; ++i)
        dyn[i] = (i < ds.dynamic_marks.size() && ds.dynamic_marks[i]) || std::find(skinned_keys.begin(), skinned_keys.end(), key(i)) != skinned_keys.end();
    std::vector<DeviceScene::Blas> blases;
    std::vector<std::vector<uint>> lists;
    std::vector<int> inst_blas(NI, -1);
    std::vector<uint> tlas_src;
    std::vector<uint> static_list;
    for (uint i = 0; i < NI; ++i) if (merge_static && !dyn[i] && ds.host_spans[i].triangle_count > 0) static_list.push_back(i);
    if (!static_list.empty()) {
        DeviceScene::Blas b = {};
        b.world = true; b.rep = static_list[0];
        for (uint i : static_list) { b.tri_count += ds.host_spans[i].triangle_count; inst_blas[i] = 0; }
        blases.push_back(b); lists.push_back(static_list); tlas_src.push_back(0xFFFFFFFFu);
    }
    std::map<std::tuple<uint, uint, uint, uint>, int> by_span;
    for (uint i = 0; i < NI; ++i) {
        if (ds.host_spans[i].triangle_count == 0 || inst_blas[i] >= 0) continue;
        auto it = by_span.find(key(i));
        if (it == by_span.end()) {
            DeviceScene::Blas b = {};
            b.world = false; b.rep = i; b.tri_count = ds.host_spans[i].triangle_count;
            it = by_span.emplace(key(i), (int)blases.size()).first;
            blases.push_back(b); lists.push_back({i});
        }
        inst_blas[i] = it->second;
        tlas_src.push_back(i);
    }
    const uint L = (uint)tlas_src.size();
    const uint tlas_slots = L > 1 ? L - 1 : L;     // a TLAS of one leaf gets a root node of its own
    size_t node_slots = tlas_slots, records = 0;
    uint n_cap = L;
    for (DeviceScene::Blas& b : blases) {
        b.node_off = (uint)node_slots; b.tri_off = (uint)records;
        b.node_slots = b.tri_count > 1 ? b.tri_count - 1 : 0;
        b.root = b.node_slots ? (int)b.node_off : ~(int)b.tri_off;
        node_slots += b.node_slots; records += b.tri_count;
        n_cap = std::max(n_cap, b.tri_count);
    }
    if (node_slots * sizeof(Bvh4Node) > 0xFFFFFFFFull) return set_error("trhip_scene_build_accel: more than 2^25 nodes");
    if (records > 0x7FFFFFF0ull) return set_error("trhip_scene_build_accel: too many triangle records");
    // outputs (kept while their sizes do not change: a rebuild allocates nothing)
    if (ds.node_capacity != node_slots || ds.tri_capacity != records || ds.tlas_capacity != L) {
        ds.free_accel();
        if (records) HIPCHK(hipMalloc(&ds.tris, records * sizeof(TriRecord)));
        // node slots, then the TLAS leaf records (SceneView finds them behind node_count: common.h tlas_leaves)
        const size_t leaf_bytes = (((size_t)L * sizeof(TlasLeaf) + sizeof(Bvh4Node) - 1) / sizeof(Bvh4Node)) * sizeof(Bvh4Node);
        if (node_slots) HIPCHK(hipMalloc(&ds.nodes4, node_slots * sizeof(Bvh4Node) + leaf_bytes));
        ds.tlas = reinterpret_cast<TlasLeaf*>(ds.nodes4 + node_slots);
        if (L) HIPCHK(hipMalloc(&ds.tlas_src_leaves, (size_t)L * sizeof(TlasLeaf)));
        ds.node_capacity = node_slots; ds.tri_capacity = records; ds.tlas_capacity = L;
    }
    ds.blases = blases; ds.inst_blas = inst_blas; ds.tlas_src = tlas_src; ds.tlas_leaf_count = L; ds.tlas_node_slots = tlas_slots;
    ds.blas_dirty.assign(blases.size(), 0); ds.static_dirty = false; ds.alpha_dirty.assign(NI, 0);
    ds.two_level = true;
    TreePlan P;
    if (int rc = plan_tree(ds, stream, n_cap, P)) return rc;
    // the instance lists of the BLASes (prefix sums of their triangle counts behind them) in the aux buffer
    size_t list_words = 0;
    for (auto& l : lists) list_words += 2 * l.size() + 1;
    if (int rc = ensure_aux(ds, list_words * 4)) return rc;
    std::vector<uint> words;
    words.reserve(list_words);
    std::vector<size_t> list_at;
    for (auto& l : lists) {
        list_at.push_back(words.size());
        words.insert(words.end(), l.begin(), l.end());
        uint acc = 0;
        words.push_back(0);
        for (uint i : l) { acc += ds.host_spans[i].triangle_count; words.push_back(acc); }
    }
    uint* aux = static_cast<uint*>(ds.tl_aux);
    if (!words.empty()) HIPCHK(hipMemcpyAsync(aux, words.data(), words.size() * 4, hipMemcpyHostToDevice, stream));
    SceneView sv = ds.view();
    sv.tri_count = ds.tri_count;
    for (size_t g = 0; g < blases.size(); ++g) {
        const DeviceScene::Blas& b = blases[g];
        const uint nl = (uint)lists[g].size();
        HIPCHK(hipMemcpyAsync(P.cbounds(), kCboundsInit, sizeof(kCboundsInit), hipMemcpyHostToDevice, stream));
        const uint blocks = (b.tri_count + BT - 1) / BT;
        hipLaunchKernelGGL(k_group_records, dim3(blocks), dim3(BT), 0, stream, sv, aux + list_at[g], aux + list_at[g] + nl, nl, b.tri_count, b.world ? 1 : 0,
                           ds.non_opaque, ds.alpha_base, ds.alpha_tris, P.unsorted());
        hipLaunchKernelGGL(k_record_bounds, dim3(blocks < 1024u ? blocks : 1024u), dim3(BT), 0, stream, b.tri_count, P.unsorted(), P.cbounds());
        if (int rc = build_tree(ds, stream, P, b.tri_count, ds.tris + b.tri_off, ds.nodes4 + b.node_off)) return rc;
        if (b.node_slots) hipLaunchKernelGGL(k_rebase, dim3((b.node_slots + BT - 1) / BT), dim3(BT), 0, stream, ds.nodes4 + b.node_off, b.node_slots, (int)b.node_off, (int)b.tri_off);
        HIPCHK(hipGetLastError());
    }
    if (ds.alpha_count && ds.tri_count)
        hipLaunchKernelGGL(k_alpha_records, dim3((ds.tri_count + BT - 1) / BT), dim3(BT), 0, stream, sv, ds.tri_prefix, ds.non_opaque, ds.alpha_base, ds.alpha_tris);
    HIPCHK(hipEventRecord(T.e[1], stream));
    if (int rc = build_tlas(ds, stream, P)) return rc;
    ds.leaf_count = (uint)records;
    ds.node_count = (uint)node_slots;
    ds.accel_tri_count = ds.tri_count;
    ds.accel_built = true;
    if (int rc = extract_tri_lights(ds, stream)) return rc;
    HIPCHK(hipEventRecord(T.e[2], stream));
    HIPCHK(hipEventSynchronize(T.e[2]));
    float ms_blas = 0, ms_tlas = 0;
    HIPCHK(hipEventElapsedTime(&ms_blas, T.e[0], T.e[1]));
    HIPCHK(hipEventElapsedTime(&ms_tlas, T.e[1], T.e[2]));
    ds.layout = {};
    ds.layout.strategy = ds.accel_strategy; ds.layout.blas_count = (uint)blases.size(); ds.layout.tlas_leaf_count = L;
    ds.layout.blas_updated = (uint)blases.size();
    ds.layout.node_bytes = (uint64_t)node_slots * sizeof(Bvh4Node);
    ds.layout.record_bytes = (uint64_t)records * sizeof(TriRecord) + (uint64_t)L * sizeof(TlasLeaf);
    ds.layout.blas_ms = ms_blas; ds.layout.tlas_ms = ms_tlas;
    fill_info(ds, info, ms_blas + ms_tlas);
    return 0;
}

// Level lists of the live nodes under `roots` (breadth-first), as refit_accel builds them for the whole tree
static int node_levels(DeviceScene& ds, hipStream_t stream, const std::vector<uint>& roots, std::vector<uint>& offsets) {
    offsets.assign(1, 0u);
    if (roots.empty()) return 0;
    const uint n1 = ds.node_count;
    if (!ds.level_nodes) HIPCHK(hipMalloc(&ds.level_nodes, (size_t)n1 * 4));
    if (!ds.node_bounds) HIPCHK(hipMalloc(&ds.node_bounds, (size_t)n1 * 24));
    uint* counter = reinterpret_cast<uint*>(ds.node_bounds);      // the bounds are written afterwards, level by level
    HIPCHK(hipMemcpyAsync(ds.level_nodes, roots.data(), roots.size() * 4, hipMemcpyHostToDevice, stream));
    uint begin = 0, count = (uint)roots.size();
    while (count > 0) {
        offsets.push_back(begin + count);
        if (begin + count >= n1) break;
        HIPCHK(hipMemsetAsync(counter, 0, 4, stream));
        hipLaunchKernelGGL(k_expand_level, dim3((count + BT - 1) / BT), dim3(BT), 0, stream, count, ds.level_nodes + begin, ds.nodes4, ds.level_nodes + begin + count, counter);
        uint next = 0;
        HIPCHK(hipMemcpyAsync(&next, counter, 4, hipMemcpyDeviceToHost, stream));
        HIPCHK(hipStreamSynchronize(stream));
        begin += count; count = next;
        if (offsets.size() > 4096) return set_error("trhip_scene_refit_accel: hierarchy too deep");
    }
    return 0;
}

static int refit_two_level(DeviceScene& ds, hipStream_t stream, trhip_accel_info* info) {
    Timer T;
    for (hipEvent_t& x : T.e) HIPCHK(hipEventCreate(&x));
    HIPCHK(hipEventRecord(T.e[0], stream));
    SceneView sv = ds.view();
    sv.tri_count = ds.tri_count;
    std::vector<uint> roots;
    uint updated = 0;
    for (size_t g = 0; g < ds.blases.size(); ++g) {
        const DeviceScene::Blas& b = ds.blases[g];
        if (!(b.world ? ds.static_dirty : ds.blas_dirty[g] != 0)) continue;
        updated++;
        const uint blocks = (b.tri_count + BT - 1) / BT;
        if (b.world) hipLaunchKernelGGL(k_retransform, dim3(blocks), dim3(BT), 0, stream, sv, b.tri_count, ds.tris + b.tri_off, ds.alpha_base, ds.alpha_tris);
        else hipLaunchKernelGGL(k_retransform_obj, dim3(blocks), dim3(BT), 0, stream, sv, b.tri_count, ds.tris + b.tri_off);
        if (b.root >= 0) roots.push_back((uint)b.root);
    }
    if (!roots.empty()) {
        std::vector<uint> offsets;
        if (int rc = node_levels(ds, stream, roots, offsets)) return rc;
        for (size_t l = offsets.size(); l-- > 1;) {
            const uint lo = offsets[l - 1], cnt = offsets[l] - lo;
            if (cnt) hipLaunchKernelGGL(k_refit_level, dim3((cnt + BT - 1) / BT), dim3(BT), 0, stream, cnt, ds.level_nodes + lo, ds.nodes4, ds.tris, ds.node_bounds);
        }
    }
    {   // the any-hit records of the non-opaque instances whose material changed or whose mesh was skinned (a rigid move touches none)
        std::vector<uint> list, prefix(1, 0u);
        for (uint i = 0; i < ds.alpha_dirty.size(); ++i)
            if (ds.alpha_dirty[i] && ds.host_spans[i].triangle_count) { list.push_back(i); prefix.push_back(prefix.back() + ds.host_spans[i].triangle_count); }
        if (!list.empty()) {
            const size_t words = list.size() + prefix.size();
            if (words > ds.alpha_list_words) {
                if (ds.alpha_list) (void)hipFree(ds.alpha_list);
                ds.alpha_list = nullptr; ds.alpha_list_words = 0;
                HIPCHK(hipMalloc(&ds.alpha_list, words * 4));
                ds.alpha_list_words = words;
            }
            list.insert(list.end(), prefix.begin(), prefix.end());
            HIPCHK(hipMemcpyAsync(ds.alpha_list, list.data(), words * 4, hipMemcpyHostToDevice, stream));
            const uint n_list = (uint)(words - 1) / 2, n = prefix.back();
            hipLaunchKernelGGL(k_alpha_list, dim3((n + BT - 1) / BT), dim3(BT), 0, stream, sv, ds.alpha_list, ds.alpha_list + n_list, n_list, n, ds.alpha_base,
                               ds.alpha_tris);
            HIPCHK(hipStreamSynchronize(stream));   // `list` lives in this block
        }
        std::fill(ds.alpha_dirty.begin(), ds.alpha_dirty.end(), 0);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(T.e[1], stream));
    uint n_cap = ds.tlas_leaf_count;
    TreePlan P;
    if (int rc = plan_tree(ds, stream, n_cap, P)) return rc;
    if (int rc = build_tlas(ds, stream, P)) return rc;
    ds.accel_built = true;
    if (int rc = extract_tri_lights(ds, stream)) return rc;
    HIPCHK(hipEventRecord(T.e[2], stream));
    HIPCHK(hipEventSynchronize(T.e[2]));
    float ms_blas = 0, ms_tlas = 0;
    HIPCHK(hipEventElapsedTime(&ms_blas, T.e[0], T.e[1]));
    HIPCHK(hipEventElapsedTime(&ms_tlas, T.e[1], T.e[2]));
    std::fill(ds.blas_dirty.begin(), ds.blas_dirty.end(), 0);
    ds.static_dirty = false;
    ds.layout.blas_updated = updated; ds.layout.blas_ms = ms_blas; ds.layout.tlas_ms = ms_tlas;
    fill_info(ds, info, ms_blas + ms_tlas);
    return 0;
}

}  // namespace tr

// =====================================================================================================================
// Sphere-light tree (trhip_scene_set_light_accel).  One box record per light with radius != 0 (v0 = lo, v1 = hi,
// v2 = lo, prim = light index), built like the TLAS by build_tree, then leaf ~j (sorted record j) renamed ~light index.  The leaf box is
// pos +- (r + TR_LIGHT_KAPPA (|pos|inf + r)), rounded outwards (trace.h: what makes the walk exact for the fp32 root).
namespace tr {

#ifndef TR_LIGHT_AUTO_THRESHOLD
#define TR_LIGHT_AUTO_THRESHOLD 16      // sphere lights from which TRHIP_LIGHT_ACCEL_AUTO walks the tree: the smallest measured count at which it
                                        // is not slower than the loop (profiles/r8/sphere_light_accel.txt)
#endif
uint light_accel_auto_threshold() { return TR_LIGHT_AUTO_THRESHOLD; }
int light_accel_requested(const DeviceScene& ds) {
    if (ds.light_accel_requested >= 0) return ds.light_accel_requested;
    const char* e = getenv("TRHIP_LIGHT_ACCEL");
    std::string v = e ? e : "";
    for (char& c : v) c = (char)tolower((unsigned char)c);
    if (v.empty() || v == "auto") return TRHIP_LIGHT_ACCEL_AUTO;
    return v == "loop" ? TRHIP_LIGHT_ACCEL_LOOP : (v == "tree" ? TRHIP_LIGHT_ACCEL_TREE : -1);
}

namespace {

void light_box(const PointLight& pl, float lo[3], float hi[3]) {
    const double p[3] = {pl.pos.x, pl.pos.y, pl.pos.z}, r = std::fabs((double)pl.radius);
    const double m = std::max(std::fabs(p[0]), std::max(std::fabs(p[1]), std::fabs(p[2])));
    const double g = r + (double)TR_LIGHT_KAPPA * (m + r);
    for (int k = 0; k < 3; ++k) {
        lo[k] = std::nextafter((float)(p[k] - g), -INFINITY);
        hi[k] = std::nextafter((float)(p[k] + g), INFINITY);
    }
}

// union of the children of `node`, written into its slots on the way (post-order); returns the node's box
void refit_light_node(std::vector<Bvh4Node>& nodes, const std::vector<PointLight>& lights, int node, float lo[3], float hi[3]) {
    for (int k = 0; k < 3; ++k) { lo[k] = INFINITY; hi[k] = -INFINITY; }
    Bvh4Node& nd = nodes[(size_t)node];
    for (int c = 0; c < 4; ++c) {
        const int ch = nd.child[c];
        if (ch == 0x7FFFFFFF) continue;
        float clo[3], chi[3];
        if (ch < 0) light_box(lights[(size_t)~ch], clo, chi);
        else refit_light_node(nodes, lights, ch, clo, chi);
        nd.lox[c] = clo[0]; nd.loy[c] = clo[1]; nd.loz[c] = clo[2]; nd.hix[c] = chi[0]; nd.hiy[c] = chi[1]; nd.hiz[c] = chi[2];
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], clo[k]); hi[k] = std::max(hi[k], chi[k]); }
    }
}

int write_light_header(DeviceScene& ds, uint use_tree) {
    const uint n = ds.point_light_count;
    const LightTreeHeader h = {use_tree, ds.light_tree_nodes, use_tree ? (uint)ds.light_tree_set.size() : 0u, 0u};
    HIPCHK(hipMemcpy(reinterpret_cast<char*>(ds.point_lights) + (size_t)n * sizeof(PointLight), &h, sizeof(h), hipMemcpyHostToDevice));
    return 0;
}

int build_light_tree(DeviceScene& ds, hipStream_t stream) {
    const uint L = (uint)ds.light_tree_set.size();
    Bvh4Node* dst = const_cast<Bvh4Node*>(light_tree_nodes(ds.view()));
    std::vector<TriRecord> recs(L);
    for (uint j = 0; j < L; ++j) {
        TriRecord& t = recs[j];
        memset(&t, 0, sizeof(t));
        float lo[3], hi[3];
        light_box(ds.host_point_lights[ds.light_tree_set[j]], lo, hi);
        for (int k = 0; k < 3; ++k) { t.v0[k] = lo[k]; t.v1[k] = hi[k]; t.v2[k] = lo[k]; }
        t.prim = ds.light_tree_set[j];
    }
    std::vector<Bvh4Node>& nodes = ds.light_nodes;
    if (L == 1) {   // the root is a node of one child, so that every walk starts at node 0
        nodes.assign(1, Bvh4Node());
        Bvh4Node& root = nodes[0];
        for (int c = 0; c < 4; ++c) {
            root.lox[c] = root.loy[c] = root.loz[c] = INFINITY; root.hix[c] = root.hiy[c] = root.hiz[c] = -INFINITY;
            root.child[c] = 0x7FFFFFFF; root.pad[c] = 0;
        }
        root.lox[0] = recs[0].v0[0]; root.loy[0] = recs[0].v0[1]; root.loz[0] = recs[0].v0[2];
        root.hix[0] = recs[0].v1[0]; root.hiy[0] = recs[0].v1[1]; root.hiz[0] = recs[0].v1[2];
        root.child[0] = ~(int)recs[0].prim;
    } else {
        const uint saved_rounds = ds.build_rounds;      // what trhip_accel_info reports is the triangle build's
        TreePlan P;
        if (int rc = plan_tree(ds, stream, L, P)) return rc;
        TriRecord* sorted = nullptr;
        HIPCHK(hipMalloc(&sorted, (size_t)L * sizeof(TriRecord)));
        HIPCHK(hipMemcpyAsync(P.unsorted(), recs.data(), (size_t)L * sizeof(TriRecord), hipMemcpyHostToDevice, stream));
        HIPCHK(hipMemcpyAsync(P.cbounds(), kCboundsInit, sizeof(kCboundsInit), hipMemcpyHostToDevice, stream));
        const uint blocks = (L + BT - 1) / BT;
        hipLaunchKernelGGL(k_record_bounds, dim3(blocks < 1024u ? blocks : 1024u), dim3(BT), 0, stream, L, P.unsorted(), P.cbounds());
        int rc = build_tree(ds, stream, P, L, sorted, dst);
        ds.build_rounds = saved_rounds;
        nodes.resize((size_t)L - 1);
        std::vector<TriRecord> order(L);
        if (rc == 0) {
            hipError_t e = hipStreamSynchronize(stream);
            if (e == hipSuccess) e = hipMemcpy(nodes.data(), dst, nodes.size() * sizeof(Bvh4Node), hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(order.data(), sorted, (size_t)L * sizeof(TriRecord), hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = set_error(std::string("light tree: ") + hipGetErrorString(e));
        }
        (void)hipFree(sorted);
        if (rc) return rc;
        for (Bvh4Node& nd : nodes)      // leaf ~j of the sorted records -> ~light index (dead slots too: harmless, never reached)
            for (int c = 0; c < 4; ++c)
                if (nd.child[c] < 0) nd.child[c] = ~(int)order[(size_t)~nd.child[c]].prim;
    }
    ds.light_tree_nodes = (uint)nodes.size();
    HIPCHK(hipMemcpy(dst, nodes.data(), nodes.size() * sizeof(Bvh4Node), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

int update_light_accel(DeviceScene& ds, bool moved) {
    const uint n = ds.point_light_count;
    std::vector<uint> set;
    for (uint i = 0; i < n; ++i) if (ds.host_point_lights[i].radius != 0.0f) set.push_back(i);
    const int requested = light_accel_requested(ds);
    if (requested < 0) return set_error(std::string("TRHIP_LIGHT_ACCEL: unknown value '") + getenv("TRHIP_LIGHT_ACCEL") + "' (auto, loop or tree)");
    const bool tree = !set.empty() && (requested == TRHIP_LIGHT_ACCEL_TREE || (requested == TRHIP_LIGHT_ACCEL_AUTO && set.size() >= light_accel_auto_threshold()));
    ds.light_in_effect = tree ? TRHIP_LIGHT_ACCEL_TREE : TRHIP_LIGHT_ACCEL_LOOP;
    if (n == 0) return 0;
    if (!tree) {
        ds.light_tree_set.clear(); ds.light_nodes.clear(); ds.light_tree_nodes = 0;
        return write_light_header(ds, 0u);
    }
    const bool current = set == ds.light_tree_set && !ds.light_nodes.empty();
    if (current && !moved) return write_light_header(ds, 1u);     // a mode change over a tree that is up to date
    const auto t0 = std::chrono::steady_clock::now();
    if (current) {      // same lights: new boxes in the same tree
        float lo[3], hi[3];
        refit_light_node(ds.light_nodes, ds.host_point_lights, 0, lo, hi);
        HIPCHK(hipMemcpy(const_cast<Bvh4Node*>(light_tree_nodes(ds.view())), ds.light_nodes.data(), ds.light_nodes.size() * sizeof(Bvh4Node), hipMemcpyHostToDevice));
        ds.light_last_refit = 1;
    } else {
        ds.light_tree_set = set;
        if (int rc = build_light_tree(ds, nullptr)) { ds.light_tree_set.clear(); ds.light_nodes.clear(); ds.light_tree_nodes = 0; (void)write_light_header(ds, 0u); return rc; }
        ds.light_last_refit = 0;
    }
    if (int rc = write_light_header(ds, 1u)) return rc;
    ds.light_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

}  // namespace tr
