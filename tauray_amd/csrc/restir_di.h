// ReSTIR DI - reservoir resampling of direct light (shader/restir_di.glsl, shader/restir_di_canonical_and_temporal.rgen,
// shader/restir_di_spatial.rgen restated; the reference's own host no longer wires these up): constants, layouts, the order of operations
// and the order of random draws of k_restir_di_canonical and k_restir_di_spatial (restir_di.hip) behind the entry points trhip_restir_di_*
// (include/trhip.h).  tests/restir_di_model.py repeats this file in float32 and float64.
//
// Layouts (all fp32 / u32 / i32, [layers][h][w] records):
//   surface record    RestirSurface, 112 bytes = seven aligned 16-byte words (the shader's `domain`, restir_di.glsl:39-46,86-99); a miss is
//                     all zero but instance_id = -1.  Two of them: frame f writes half f & 1 and reads the other as the previous frame's.
//   reservoir         RestirReservoir, 32 bytes = two aligned 16-byte words: uc_weight, target_function, light_type << 30 | light_index,
//                     confidence, light_data.xy, two zero words (write_reservoir_buffer, restir_di.glsl:411-425).  The null sample is
//                     type 0 with index (1u << 30) - 1.  `canonical` is written by the canonical kernel and read by the spatial one,
//                     `history` is written by the spatial kernel and read by the next frame's canonical kernel.
//   decision records  (options.record) RestirCandidateRecord [pixel][candidates], RestirTemporalRecord [pixel], RestirSpatialRecord
//                     [pixel][spatial_samples], RestirFinalRecord [pixel]
//
// Random draws.  sampler = init_local_sampler((px, py, viewport, 0), 2 * frame + pass, pcg(rng_seed) or 0, uniform) (rng.h), pass = 0 in
// the canonical kernel and 1 in the spatial one, frame = the stage's frame counter: two disjoint streams (the shaders seed both passes
// alike).  A draw is pcg4d(sampler.rs); "unit" = float(word) * 2^-32 per component.  Order:
//   canonical  [TEMPORAL: one draw, unit .xy: the reprojection]  per candidate: one draw (the four words: sample_canonical), one draw
//              (unit .x: the selection)  [reuse: one draw, unit .x: the temporal merge]
//   spatial    2 * SPATIAL draws (unit .xy: the offsets), per slot that holds a neighbour whose sample is not null one draw (unit .x),
//              one draw (unit .x: the canonical merge)
//
// Order of operations (plain fp32, no contraction, correctly rounded divide and square root; dot(a, b) = a.x * b.x + a.y * b.y + a.z * b.z
// left to right; the functions named are those of shading.h with RoundedMath (common.h) for their sin, cos, pow and atan2: the double
// function of the float argument rounded once, so that the model has the kernels' bits; the first hit is shaded as every stage shades it):
//   surface      v, mat = shade_surface of the first hit (k_gbuffer's front half);  view = normalize(v.pos - ray origin);
//                flat_normal = v.hard_normal
//   contribution light_contribution (restir_di.glsl:155-249) of sample (type, index, data) at a surface:
//                point      to = pl.pos - pos; dir = normalize(to); dist2 = dot(to, to); normal = 0;
//                           colour = (pl.color * get_spotlight_intensity(pl, dir)) / max(dist2, 1e-7f)
//                triangle   A, B, C = tl.pos[k] - pos;  p = (data.x * A + data.y * B) + (1.0f - data.x - data.y) * C;  dir = normalize(p);
//                           dist2 = dot(p, p);  normal = normalize(cross(tl.pos[2] - tl.pos[0], tl.pos[1] - tl.pos[0]));
//                           colour = r9g9b9e5_to_rgb(emission_factor), 0 when |dot(dir, normal)| < 0.001f, times the emission texture at
//                           (data.x * uv0 + data.y * uv1) + b.z * uv2 when there is one
//                directional dir = sample_cone(data, -dl.dir, dl.dir_cutoff);  dist2 = inf;
//                           colour = dl.dir_cutoff >= 1 ? dl.color : dl.color * (1.0f / (2.0f * pi * (1.0f - dl.dir_cutoff)))
//                environment dir = uv_to_latlong_direction(data);  dist2 = inf;  colour = environment_factor.rgb * sample_envmap(data).rgb
//                then: dot(dir, flat_normal) < 1e-6f gives 0;  tbn = create_tangent_space(mapped_normal);
//                shading_view = view_to_tangent_space(view, tbn) (z clamped to 1e-5f);  shading_light = dir * tbn;
//                lobes = 0; ggx_bsdf_pdf(shading_light, shading_view, mat, lobes); correct_lobes_for_normal_map(dir, flat_normal, lobes);
//                value = modulate_bsdf(mat, lobes) * colour;  a NaN in data gives 0.  The null sample, or an index past the current
//                frame's light count of its type, gives 0 with dir = 0, dist2 = 0 and no shadow ray.
//   visibility   a contribution with a component > 0 casts trace_shadow4(pos, dir, min_ray_dist, sqrtf(dist2) - min_ray_dist); any other
//                casts none and has visibility 0.  target = rgb_to_luminance(contribution * visibility)
//   candidates   sample_canonical (restir_di.glsl:251-354) with u = unit(draw): classes in the order point, triangle, directional,
//                environment by `(u.w -= prob) < 0` with the scene's NEE probabilities (nee_probabilities, pt.h; all four weights 1);
//                point: index = clamp(int(u.x * n), 0, n - 1), pdf = (1.0f / n) * prob;  triangle: index from u.z,
//                dir = sample_triangle_light(solid angle, u.xy, A, B, C, tri_pdf), len = ray_plane_intersection_dist(dir, A, B, C),
//                tri_pdf = 1e9f when it is inf, <= 0, len <= min_ray_dist or dir has a NaN, data = get_barycentric_coords(dir * len, A, B, C).xy,
//                pdf = (tri_pdf * (1.0f / n)) * prob;  directional: index from u.z, data = u.xy,
//                pdf = ((cutoff >= 1 ? 1.0f : 1.0f / (2.0f * pi * (1.0f - cutoff))) / n) * prob;  environment: the alias table as
//                sample_environment_map (shade_kernel.h) reads it, data = (pixel + off) / size, pdf = entry pdf * prob;  no class taken
//                (no lights, or u.w past the sum by rounding): the null sample with pdf 1.
//                weight = (1.0f / (float(candidates) + prev_confidence)) * target / pdf, NaN -> 0;  update_reservoir:
//                weight_sum += weight; selected = u * weight_sum < weight (then the reservoir takes sample and target);  confidence += 1
//                after the loop uc_weight = weight_sum > 0 ? weight_sum / target : 0
//   light selection (trhip_restir_di_set_light_selection; uniform, the default, is `candidates` above word for word; power, decisions 23 to 28
//                of trhip.h, changes how the index of a point or triangle candidate is drawn and what its pdf is, nothing else):
//                weights   fp32, one per light (k_restir_light_weights, restir_di_power.hip): point or spot light rgb_to_luminance(color) -
//                          the spot cone and the radius are ignored; triangle light rgb_to_luminance(r9g9b9e5_to_rgb(emission_factor)) *
//                          (0.5f * length(cross(pos[1] - pos[0], pos[2] - pos[0]))) - the emission texture is ignored; a weight that is
//                          negative, NaN or infinite is 0.  Directional lights, the environment and the class probabilities keep their rule.
//                pdf       inside a class of n lights p_i = (1 - f) * w_i / sum(w) + f / n in double (sum: one running double sum in
//                          slot order), f = uniform_fraction in (0, 1]; 1 / n when sum(w) = 0.  The uniform share keeps the estimator
//                          unbiased where the weight is blind (textures, cones, a table that is stale because lights moved since it was
//                          built): a light that contributes has a positive pdf.
//                table     one AliasEntry per light, the point lights' table then the triangle lights', each over its own n slots, built on
//                          the host (include/tauray_alias.hh) from n * p_i in the work-list order and the threshold encoding of the
//                          environment map's table; the steps are doubles, not floats: a float n * p_i is off by up to 2^-25 relative, and
//                          the thresholds are asked to reproduce p_i to 2^-30.  pdf / alias_pdf = float(p_i) of the slot and of its alias.
//                draw      point: p = uint64(rnd.x) * n, slot = p >> 32, low = uint32(p); e = table[slot], one 16-byte load ahead of the
//                          light record's; low > e.probability: index = e.alias_id, pdf = e.alias_pdf, else index = slot, pdf = e.pdf;
//                          light_pdf = pdf * prob_point.  triangle: the same with rnd.z and the table's second part,
//                          light_pdf = (tri_pdf * pdf) * prob_tri; u.xy still place the point on the triangle.  No draw is added or
//                          removed, the streams stay where they are.  Limit: a light's frequency differs from its recorded pdf by at most
//                          n / 2^32 relative, the granularity of `low` and of the slot.
//                The pdf enters only the candidate weight target / pdf: the merges, the Jacobians, the MIS terms and the reservoirs never
//                see it, so the table may be rebuilt while there is history (trhip_restir_di_refresh_light_selection); mode and fraction
//                change only without history.  ReSTIR GI's light sample at a secondary hit (restir_gi.hip) stays uniform.
//   bsdf candidates (trhip_restir_di_set_bsdf_candidates; decisions 29 to 36 of trhip.h; k_restir_di_canonical_bsdf, restir_di_bsdf.hip;
//                L = candidates, B = bsdf_candidates in 0..8, L + B <= 32, M = L + B; B = 0, the default, is `candidates` word for word
//                and the kernels that were; with B > 0 the L light candidates are drawn as above, then the B BSDF candidates):
//                1 draws     per BSDF candidate, null or not: one draw (the four unit words: ggx_bsdf_sample's ur), one draw (unit .x: the
//                            selection).  The temporal merge's draw follows.
//                2 direction tbn = create_tangent_space(mapped_normal), shading_view = view_to_tangent_space(view, tbn), mat: as
//                            `contribution`;  ggx_bsdf_sample<RoundedMath>(ur, shading_view, mat, out_dir, ..);  dir = normalize(tbn * out_dir)
//                3 p_b       p_b(surface, dir) = the value of ggx_bsdf_pdf<RoundedMath>(dir * tbn, shading_view, mat, lobes), for candidates of
//                            both techniques.  The pdf ggx_bsdf_sample returns is not used.
//                4 null      out_dir has a NaN or is 0; p_b is not > 0 (zero roughness: mirrors gain nothing); dot(dir, flat_normal) < 1e-6f:
//                            the null sample, weight 0, nothing traced.
//                5 ray       trace_closest4<1, false, TWO_LEVEL>(pos, dir, min_ray_dist, inf).  Hit, instance.light_base_id >= 0 and
//                            index = light_base_id + primitive < tri_light_count: (type 1, index, data = (1.0f - u - v, u)).  Miss and an
//                            environment: (type 3, 0, data = (atan2(dir.z, dir.x) / (2.0f * pi) + 0.5f,
//                            atan2(-dir.y, sqrtf(dir.x * dir.x + dir.z * dir.z)) / pi + 0.5f)).  Anything else: the null sample.
//                6 value     restir_fetch_light, `contribution` as for any sample; visibility = 1 where the contribution has a component
//                            > 0, else 0, in every visibility mode: no shadow ray.  Limit: an environment sample's direction is rebuilt
//                            from its uv and differs from the traced one by rounding.
//                7 p_l       light candidate: its pdf above.  Found triangle: A, B, C = tl.pos[k] - pos; the solid angle of
//                            sample_spherical_triangle operation for operation (nA .. G2, solid = 2.0f * atan2(G0, G1 + G2));
//                            tri_pdf = 1.0f / solid; len = ray_plane_intersection_dist(contribution's dir, A, B, C); tri_pdf = 1e9f when it
//                            is inf, <= 0, len <= min_ray_dist or dir has a NaN;  sel = 1.0f / float(n_tri), power selection:
//                            table[n_point + index].pdf;  p_l = (tri_pdf * sel) * prob_tri.  Found environment sample:
//                            pixel = clamp(int(floorf(data * size)), 0, size - 1) per axis; p_l = alias_table[pixel].pdf * prob_env.
//                            A class of probability 0, or an invalid sample: 0.
//                8 p_b of a light candidate: types 0 and 2: 0; types 1 and 3: item 3 at the contribution's dir.
//                9 weight    denom = float(L) * p_l + float(B) * p_b (two products, one sum);  mis = float(M) / (float(M) + prev_confidence);
//                            weight = (mis * target) / denom;  NaN, or not denom > 0: 0.  update_reservoir, confidence += 1 as above.
//                            After the loops everything is as above.
//                The pdfs enter only the candidate weight; B changes only without history.  Rays a pixel: B closest-hit rays more in
//                every visibility mode.  Records: the candidate record's pdf is p_l; RestirBsdfRecord (restir_di_bsdf.h) next to it.
//   sphere lights (trhip_restir_di_set_sphere_lights; decisions 37 to 44 of trhip.h; restir_di_sphere.h, restir_di_sphere.hip; point, the
//                default, is everything above word for word and the kernels that were; area: a type-0 sample whose light has
//                radius != 0 is a point on that sphere; a light of radius 0 is what it was, in both modes):
//                1 sample    type 0 and the index stay; light_data = the octahedral encoding of the outward unit normal n of the point.
//                            encode: s = |n.x| + |n.y| + |n.z|; p = (n.x / s, n.y / s); n.z < 0: p = ((1.0f - |p.y|) * sign(p.x),
//                            (1.0f - |p.x|) * sign(p.y)) with sign(v) = v >= 0 ? 1 : -1.  decode: n = (p.x, p.y, (1.0f - |p.x|) - |p.y|);
//                            t = max(-n.z, 0); n.x += n.x >= 0 ? -t : t, likewise n.y; normalize(n).  No transcendental function.
//                            The point is fixed in the world: a neighbour or the next frame evaluates the same sample.
//                2 draw      behind restir_sample_canonical or restir_sample_canonical_power, for a type-0 sample with radius != 0
//                            (restir_sphere_draw; u.x chose the index, u.y and u.z are free): d = pos - pl.pos; dist2 = dot(d, d);
//                            k = 1.0f - r * r / dist2; cutoff = k > 0 ? sqrtf(k) : -1; dir = sample_cone((u.y, u.z), -normalize(d), cutoff);
//                            b = dot(d, dir); len = -b - sqrtf(max(b * b - dist2 + r * r, 0)); x = pos + dir * len;
//                            n = normalize(x - pl.pos); data = encode(n); solid_pdf = 1 / (2.0f * pi * (1.0f - cutoff));
//                            solid_pdf = 1e9f when n has a NaN or len <= min_ray_dist; light_pdf = (the sampler's light_pdf) * solid_pdf.
//                            No draw is added or removed.
//                3 contribution (type 0, radius != 0): n = decode(data); x = pl.pos + r * n; p = x - pos; dir = normalize(p);
//                            dist2 = dot(p, p); normal = n;
//                            colour = (pl.color * get_spotlight_intensity(pl, normalize(pl.pos - pos))) / (r * r * pi), 0 when
//                            dot(n, dir) >= 0 (the point faces away, or the receiver is inside the sphere; written !(dot < 0), so that
//                            the NaN of a point that is the receiver itself gives 0 too).  The candidate's own
//                            contribution is evaluated from data like every other.  Everything behind the colour is unchanged.
//                4 jacobian, visibility, merges: unchanged code; normal != 0 gives the solid-angle ratio, the shadow ray ends
//                            min_ray_dist short of x, shadow rays do not see lights.
//                5 power selection: the weights ignore the radius.  6 bsdf candidates: a BSDF ray does not return a sphere light,
//                            type-0 samples keep p_b = 0; unbiased, the light technique covers the whole visible cap.
//                Limits: ReSTIR GI's own light sample at a secondary hit stays a point; the camera ray does not see sphere lights.
//                A reservoir does not mix two meanings of light_data: the mode changes only while the stage holds no history.
//   reprojection m = get_camera_projection(previous camera, surface_prev_pos).xy;  m.y = 1.0f - m.y;  m = m * size - 0.5f;  im = int(m)
//                (truncation);  off = m - float(im);  pixel = im + (off.x < u.x ? 0 : 1, off.y < u.y ? 0 : 1)   (restir_di.glsl:138-153)
//   reuse        there is history, the pixel is on screen, and not (dot(prev.mapped_normal, mapped_normal) < 0.95f or
//                length(pos - prev.pos) > 0.01f * length(origin - pos) / (|dot(view, mapped_normal)| + 0.001f))   (:375-388)
//                prev_confidence = reuse ? history.confidence : 0
//   temporal     target' = luminance(contribution of the history sample here), no shadow ray;
//                weight = ((prev.confidence / (confidence + prev.confidence)) * target') * prev.uc_weight, NaN -> 0;  update_reservoir;
//                confidence += prev.confidence;  uc_weight as above;  with TEMPORAL always confidence = min(confidence, max_confidence)
//   neighbours   offset = floorf(search_radius * sample_blackman_harris_concentric_disk(u.xy) + 0.5f) per component;  candidates off screen
//                or without a surface are passed over;  inv = 1.0f / (min(|2 proj_inverse[0][0]|, |2 proj_inverse[1][1]|) *
//                |dot(view_inverse[2].xyz, view_inverse[3].xyz - pos)|);  good = clamp(1.0f - |dot(flat_normal, npos - pos)| * inv, 0, 1) >= 0.99f
//                and dot(nflat, flat_normal) >= 0.75f;  good ones fill slots from the front while fewer than SPATIAL are held, bad ones from
//                the back while good + bad < SPATIAL (restir_di_spatial.rgen:104-130)
//   spatial      total = canonical.confidence + the held neighbours' confidences in slot order;  canonical_m = canonical.confidence / total;
//                per held slot, in order: the neighbour's sample, if not null, is re-evaluated here with a shadow ray (target_n),
//                j = type > 1 ? 1 : reconnection_jacobian(npos, x, normal, pos, x, normal) with x = pos + dir * sqrtf(dist2);
//                m = mis_noncanonical(c.conf, n.conf, total, n.target_function, target_n, j);  wi = ((target_n * m) * n.uc_weight) * j, NaN -> 0;
//                update_reservoir;  confidence += n.confidence;  then, if the canonical sample is not null, it is evaluated at the
//                neighbour's surface with a shadow ray (target_c), jc the Jacobian the other way round, and
//                canonical_m += mis_canonical(c.conf, n.conf, total, c.target_function, target_c, jc)
//                wi = (canonical_m * c.target_function) * c.uc_weight, NaN -> 0;  update_reservoir;  confidence += c.confidence;
//                uc_weight = weight_sum > 0 ? weight_sum / target : 0.  SPATIAL = 0: the canonical reservoir as it is.
//   jacobian     q = prev_src - dst, r = cur_src - dst;  (|dot(n, r)| * (lq * lq * lq)) / (|dot(n, q)| * (lr * lr * lr)) with lq = length(q),
//                lr = length(r);  1 for n = 0;  0 when inf or NaN   (restir_di.glsl:477-501)
//   colour       contribution of the chosen sample here times its shadow ray's visibility;
//                out = (contribution * uc_weight + emission, 1);  a pixel without a surface: the null reservoir and the direct stage's
//                miss colour (k_direct: the visible directional lights in order, then the environment)
//
// Visibility modes (trhip_restir_di_set_visibility; the shaders' SHARED_VISIBILITY and SAMPLE_VISIBILITY, the visibility reuse of Bitterli
// et al. 2020; a template parameter of both kernels).  Mode 0, per-target, is everything above: candidates + 2 * SPATIAL + 1 shadow rays
// a pixel.  Mode 1, shared: one ray, the chosen sample's shading.  Mode 2, sampled: two, the sample the candidates chose and the shading.
//   1 candidates   modes 1 and 2: the loop traces nothing.  The factor of the target, which is also the candidate record's `visibility`,
//                  is 1 where `visibility` above would cast a ray (the contribution has a component > 0) and 0 otherwise, so
//                  target = rgb_to_luminance(contribution * visibility) describes every mode.  Weights, draws, their order and
//                  update_reservoir are unchanged; no mode adds or removes a draw.
//   2 sampled      mode 2, behind uc_weight = restir_uc_weight(r) and ahead of the temporal merge
//                  (restir_di_canonical_and_temporal.rgen:115-122): the reservoir's sample is evaluated once more at the pixel's surface
//                  (the loop keeps neither direction nor distance; the same inputs give the same bits) and one shadow ray is cast as
//                  `visibility` says - none, and 0, for the null sample or a contribution without a positive component - then
//                  uc_weight = uc_weight * visibility.  The `sampled` record holds that visibility and the weight ahead of the multiply;
//                  in modes 0 and 1 visibility is 1, no ray; in mode 0 nothing is multiplied either, the record is (1, 0) on every
//                  pixel and the host writes it (the mode-0 kernels are the code they were).  A pixel without a surface:
//                  (mode 2 ? 0 : 1, 0).
//   3 temporal     unchanged in every mode: it never traced.
//   4 neighbours   modes 1 and 2: a bad neighbour takes no slot (restir_di_spatial.rgen:123-129 is compiled out), only the first
//                  SPATIAL good ones are held, in draw order.  The 2 * SPATIAL offset draws stay.
//   5 spatial      modes 1 and 2: neither re-evaluation traces; the factor and visibility_n / visibility_c follow point 1.
//   6 colour       the shadow ray stays in every mode.  Mode 2 (restir_di_spatial.rgen:266-269,281): uc_weight = uc_weight * visibility
//                  ahead of the history store, out = ((contribution * visibility) * uc_weight + emission, 1) with that multiplied weight.
//                  Limit: under a partly transparent occluder (0 < visibility < 1) mode 2 counts the factor once per pass that traced
//                  it; it is exact for opaque occluders only, where visibility * visibility = visibility.
//   7 bias         mode 1 is unbiased like mode 0: a target without visibility is still a valid target (positive wherever the
//                  integrand is), and the one traced ray is in the integrand.  Mode 2 is BIASED wherever visibility differs between the
//                  pixels that share a sample: a sample zeroed at the pixel that drew it is lost to neighbours and later frames that
//                  would have seen the light.  It is the paper's biased variant.
//   8 ReSTIR GI    does not change: restir_spatial_merge's SHARED_VISIBILITY parameter defaults to false, the code as it was.
// A reservoir does not mix the samples of two target functions: the mode changes only while the stage holds no history.
//
// Where the code is.  The sections reprojection, reuse, temporal, neighbours, spatial and jacobian, update_reservoir, visibility, the
// surface record and the temporal, spatial and final decision records: restir_resample.h, once for this stage and ReSTIR GI.  Here:
// the reservoir, the candidate record, sample_canonical, light_contribution and RestirDiKind, what restir_resample.h asks of a sample.
// candidates, the miss colour and the emission of `colour`: the kernels (restir_di.hip).
#pragma once
#include "restir_resample.h"

namespace tr {

constexpr uint RESTIR_NULL_INDEX = (1u << 30) - 1u;
constexpr int RESTIR_MAX_CANDIDATES = 32;
constexpr int RESTIR_MAX_BSDF_CANDIDATES = 8;      // `bsdf candidates`; light and BSDF candidates together: RESTIR_MAX_CANDIDATES

struct alignas(16) RestirReservoir {     // trhip_restir_di_reservoir
    float uc_weight, target_function; uint light; float confidence;
    f2 light_data; uint pad0, pad1;
};
struct RestirCandidateRecord {           // trhip_restir_di_candidate
    uint light; f2 light_data; float pdf;
    f3 contribution; float visibility;   // the unshadowed contribution
    float weight, draw; uint selected, pad;
};
struct alignas(16) RestirSampledRecord { // trhip_restir_di_sampled
    float visibility, uc_weight_before;  // `visibility modes` point 2: the ray of the candidates' choice and the weight it multiplied
    uint pad0, pad1;
};
static_assert(sizeof(RestirReservoir) == 32 && sizeof(RestirCandidateRecord) == 48 && sizeof(RestirSampledRecord) == 16, "layout");

struct RestirSample { uint type, index; f2 data; };
TR_DEV RestirSample restir_null_sample() { return {0u, RESTIR_NULL_INDEX, F2(0.0f)}; }

// A light's record as sample_explicit_light (shade_kernel.h) fetches it: the kind and the record are decided first, then one masked fetch
// per kind into the same four registers; the branches behind it only compute.  An environment sample has no record (the candidate
// sampler fetches its alias entry into r0 itself).  valid: not the null sample, and the index is inside the current frame's array.
struct RestirLightRecord { u4 r0, r1, r2, r3; bool valid; };
TR_DEV RestirLightRecord restir_fetch_light(const SceneView& sv, const RestirSample& s) {
    RestirLightRecord L;
    L.r0 = u4{0u, 0u, 0u, 0u}; L.r1 = L.r0; L.r2 = L.r0; L.r3 = L.r0;
    const uint n_point = sv.point_light_count, n_tri = sv.tri_light_count, n_dir = sv.directional_light_count;
    int kind = s.type == 0u ? (s.index < n_point ? 1 : 0) : s.type == 1u ? (s.index < n_tri ? 2 : 0) : s.type == 2u ? (s.index < n_dir ? 3 : 0)
                                                                                                                   : (sv.environment_proj >= 0 ? 4 : 0);
    asm volatile("" : "+v"(kind));       // as sample_explicit_light: keeps the fetches out of the tests above
    if (kind == 1) { const u4* rec = reinterpret_cast<const u4*>(sv.point_lights + s.index); L.r0 = rec[0]; L.r1 = rec[1]; L.r2 = rec[2]; L.r3 = rec[3]; }
    if (kind == 2) { const u4* rec = reinterpret_cast<const u4*>(sv.tri_lights + s.index); L.r0 = rec[0]; L.r1 = rec[1]; L.r2 = rec[2]; L.r3 = rec[3]; }
    if (kind == 3) { const u4* rec = reinterpret_cast<const u4*>(sv.directional_lights + s.index); L.r0 = rec[0]; L.r1 = rec[1]; }
    L.valid = kind != 0;
    return L;
}

// `sphere lights` 1: the octahedral map of a unit vector and back
TR_DEV f2 restir_oct_encode(f3 n) {
    const float s = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);
    f2 p = F2(n.x / s, n.y / s);
    if (n.z < 0.0f) p = F2((1.0f - fabsf(p.y)) * (p.x >= 0.0f ? 1.0f : -1.0f), (1.0f - fabsf(p.x)) * (p.y >= 0.0f ? 1.0f : -1.0f));
    return p;
}
TR_DEV f3 restir_oct_decode(f2 p) {
    f3 n = F3(p.x, p.y, (1.0f - fabsf(p.x)) - fabsf(p.y));
    const float t = fmax2(-n.z, 0.0f);
    n.x += n.x >= 0.0f ? -t : t;
    n.y += n.y >= 0.0f ? -t : t;
    return normalize(n);
}

// light_contribution (restir_di.glsl:155-249), the BSDF as the direct stage's light sample gets it (k_direct, path_tracer.hip).
// SPHERE: `sphere lights` 3; false, the default, is the code as it was.
template <bool SPHERE = false>
TR_DEV f3 restir_contribution(const SceneView& sv, const RestirSample& s, const RestirLightRecord& L, const RestirDomain& dom, f3& dir, float& dist2, f3& normal) {
#define TR_F(x) __uint_as_float(x)
    dir = F3(0.0f); dist2 = 0.0f; normal = F3(0.0f);
    if (!L.valid) return F3(0.0f);
    f3 light_color = F3(0.0f);
    if (s.type == 0u) {
        PointLight pl;
        pl.color = F3(TR_F(L.r0.x), TR_F(L.r0.y), TR_F(L.r0.z)); pl.dir = F3(TR_F(L.r0.w), TR_F(L.r1.x), TR_F(L.r1.y)); pl.pos = F3(TR_F(L.r1.z), TR_F(L.r1.w), TR_F(L.r2.x));
        pl.radius = TR_F(L.r2.y); pl.dir_cutoff = TR_F(L.r2.z); pl.dir_falloff = TR_F(L.r2.w);
        const f3 to_light = pl.pos - dom.pos;
        if (SPHERE && pl.radius != 0.0f) {
            const f3 n = restir_oct_decode(s.data);
            const f3 p = (pl.pos + pl.radius * n) - dom.pos;
            dir = normalize(p);
            dist2 = dot(p, p);
            normal = n;
            light_color = (pl.color * get_spotlight_intensity<RoundedMath>(pl, normalize(to_light))) / (pl.radius * pl.radius * TR_PI);
            if (!(dot(n, dir) < 0.0f)) light_color = F3(0.0f);      // >= 0, or a NaN: the point is the receiver itself
        } else {
            dir = normalize(to_light);
            dist2 = dot(to_light, to_light);
            light_color = (pl.color * get_spotlight_intensity<RoundedMath>(pl, dir)) / fmax2(dist2, 1e-7f);
        }
    } else if (s.type == 1u) {
        const f3 P0 = F3(TR_F(L.r0.x), TR_F(L.r0.y), TR_F(L.r0.z)), P1 = F3(TR_F(L.r0.w), TR_F(L.r1.x), TR_F(L.r1.y)), P2 = F3(TR_F(L.r1.z), TR_F(L.r1.w), TR_F(L.r2.x));
        const f3 A = P0 - dom.pos, B = P1 - dom.pos, C = P2 - dom.pos;
        const float bz = 1.0f - s.data.x - s.data.y;
        const f3 p = (s.data.x * A + s.data.y * B) + bz * C;
        dir = normalize(p);
        dist2 = dot(p, p);
        normal = normalize(cross(P2 - P0, P1 - P0));
        f3 color = r9g9b9e5_to_rgb(L.r2.y);
        if (fabsf(dot(dir, normal)) < 0.001f) color = F3(0.0f);
        const int emission_tex_id = (int)L.r3.w;
        if (emission_tex_id >= 0) {
            const f2 uv = (s.data.x * unpack_half2x16(L.r3.x) + s.data.y * unpack_half2x16(L.r3.y)) + bz * unpack_half2x16(L.r3.z);
            color = color * F3(sample_texture(sv, emission_tex_id, uv));
        }
        light_color = color;
    } else if (s.type == 2u) {
        const f3 dl_color = F3(TR_F(L.r0.x), TR_F(L.r0.y), TR_F(L.r0.z)), dl_dir = F3(TR_F(L.r1.x), TR_F(L.r1.y), TR_F(L.r1.z));
        const float dir_cutoff = TR_F(L.r1.w);
        dist2 = __builtin_huge_valf();
        dir = sample_cone<RoundedMath>(s.data, -dl_dir, dir_cutoff);
        light_color = dir_cutoff >= 1.0f ? dl_color : dl_color * (1.0f / (2.0f * TR_PI * (1.0f - dir_cutoff)));
    } else {
        dir = uv_to_latlong_direction<RoundedMath>(s.data);
        dist2 = __builtin_huge_valf();
        light_color = F3(sv.environment_factor) * F3(sample_envmap(sv, s.data));
    }
#undef TR_F
    if (dot(dir, dom.flat_normal) < 1e-6f) return F3(0.0f);
    const m3 tbn = create_tangent_space(dom.mapped_normal);
    const f3 shading_view = view_to_tangent_space(dom.view, tbn);
    const f3 shading_light = mulT(dir, tbn);
    Lobes lobes = {0, 0, 0, 0};
    ggx_bsdf_pdf<RoundedMath>(shading_light, shading_view, dom.mat, lobes);
    if (dot(dom.flat_normal, dir) < 0) { lobes.diffuse = 0; lobes.dielectric_reflection = 0; lobes.metallic_reflection = 0; }     // correct_lobes_for_normal_map
    else lobes.transmission = 0;
    f3 value = modulate_bsdf(dom.mat, lobes) * light_color;
    if (isnan(s.data.x) || isnan(s.data.y)) value = F3(0.0f);
    return value;
}

// What restir_resample.h asks of a sample: a light sample (type, index, data).  SPHERE: `sphere lights`, the area mode's meaning of a
// type-0 sample's data; RestirDiKind, the point mode, is what every kernel outside restir_di_sphere.hip is written over.
template <bool SPHERE>
struct RestirDiKindT {
    using Sample = RestirSample;
    using State = RestirState<Sample>;
    using Reservoir = RestirReservoir;
    struct Eval { f3 dir; float dist2; f3 normal; };
    // The spatial merge reads a neighbour's surface behind the first traversal: at 256 VGPRs the kernels spill less
    static constexpr bool SURFACE_LATE = true;
    static TR_DEV State create() { return {restir_null_sample(), 0.0f, 0.0f, 0.0f, 0.0f}; }
    static TR_DEV State load(const Reservoir* src) {                                           // read_reservoir_buffer (:427-454)
        const u4 a = restir_word(src, 0), b = restir_word(src, 1);
        State r;
        r.uc_weight = __uint_as_float(a.x); r.target_function = __uint_as_float(a.y);
        r.s.type = a.z >> 30; r.s.index = a.z & 0x3FFFFFFFu;
        r.confidence = __uint_as_float(a.w);
        r.s.data = F2(__uint_as_float(b.x), __uint_as_float(b.y));
        r.weight_sum = 0.0f;
        return r;
    }
    static TR_DEV void store(Reservoir* dst, const State& r) {                                 // write_reservoir_buffer (:411-425)
        restir_set_word(dst, 0, u4{TR_U(r.uc_weight), TR_U(r.target_function), r.s.type << 30 | r.s.index, TR_U(r.confidence)});
        restir_set_word(dst, 1, u4{TR_U(r.s.data.x), TR_U(r.s.data.y), 0u, 0u});
    }
    static TR_DEV float confidence(const Reservoir* src) { return __uint_as_float(restir_word(src, 0).w); }
    static TR_DEV bool is_null(const Sample& s) { return s.type == 0u && s.index == RESTIR_NULL_INDEX; }
    // the light's record is fetched per evaluation, not held across the spatial merge's loop
    static TR_DEV f3 contribution(const SceneView& sv, const Sample& s, const RestirDomain& dom, Eval& e) {
        const RestirLightRecord L = restir_fetch_light(sv, s);
        return restir_contribution<SPHERE>(sv, s, L, dom, e.dir, e.dist2, e.normal);
    }
    // the reconnection point is where the shadow ray ends; a directional or environment sample has none
    static TR_DEV float jacobian(const Sample& s, const Eval& e, f3 from, f3 at) {
        const f3 x = at + e.dir * sqrtf(e.dist2);
        return s.type > 1u ? 1.0f : restir_jacobian(from, at, x, e.normal);
    }
};
using RestirDiKind = RestirDiKindT<false>;

// sample_canonical (restir_di.glsl:251-354): select, fetch, compute, as sample_explicit_light.  The record stays in L for the contribution.
// Params: the kernel parameters of the stage that draws (prob_point, prob_tri, prob_dir, prob_env: nee_probabilities; min_ray_dist) -
// ReSTIR DI at a pixel's surface, ReSTIR GI (restir_gi.hip) at the secondary hit.
template <class Params>
TR_DEV RestirSample restir_sample_canonical(const SceneView& sv, const Params& P, u4 rnd, f3 pos, RestirLightRecord& L, float& light_pdf) {
    f4 u = u4_to_unit(rnd);
    enum { NONE = 0, POINT, TRI, DIR, ENV };
    int kind = NONE;
    if ((u.w -= P.prob_point) < 0) kind = POINT;
    else if ((u.w -= P.prob_tri) < 0) kind = TRI;
    else if ((u.w -= P.prob_dir) < 0) kind = DIR;
    else if ((u.w -= P.prob_env) < 0) kind = ENV;
    const int n_point = (int)sv.point_light_count, n_tri = (int)sv.tri_light_count, n_dir = (int)sv.directional_light_count;
    // a class with probability > 0 has lights (nee_probabilities); the counts are tested all the same, no fetch goes past an array
    if ((kind == POINT && n_point <= 0) || (kind == TRI && n_tri <= 0) || (kind == DIR && n_dir <= 0) || (kind == ENV && sv.environment_proj < 0)) kind = NONE;
    asm volatile("" : "+v"(kind));
    const int light_count = kind == POINT ? n_point : kind == TRI ? n_tri : n_dir;
    const int light_index = clampi((int)((kind == POINT ? u.x : u.z) * light_count), 0, light_count - 1);
    L.r0 = u4{0u, 0u, 0u, 0u}; L.r1 = L.r0; L.r2 = L.r0; L.r3 = L.r0;
    int alias_i = 0;
    if (kind == POINT) { const u4* rec = reinterpret_cast<const u4*>(sv.point_lights + light_index); L.r0 = rec[0]; L.r1 = rec[1]; L.r2 = rec[2]; L.r3 = rec[3]; }
    if (kind == TRI) { const u4* rec = reinterpret_cast<const u4*>(sv.tri_lights + light_index); L.r0 = rec[0]; L.r1 = rec[1]; L.r2 = rec[2]; L.r3 = rec[3]; }
    if (kind == DIR) { const u4* rec = reinterpret_cast<const u4*>(sv.directional_lights + light_index); L.r0 = rec[0]; L.r1 = rec[1]; }
    u4 alias = {0u, 0u, 0u, 0u};
    if (kind == ENV) {
        const uint sx = sv.env_w, sy = sv.env_h;
        const uint ipx = clampu(rnd.x / (0xFFFFFFFFu / sx), 0u, sx - 1u), ipy = clampu(rnd.y / (0xFFFFFFFFu / sy), 0u, sy - 1u);
        alias_i = (int)(ipx + ipy * sx);
        alias = *reinterpret_cast<const u4*>(sv.alias_table + alias_i);
    }
    L.valid = kind != NONE;
#define TR_F(x) __uint_as_float(x)
    RestirSample s = restir_null_sample();
    light_pdf = 1.0f;
    if (kind == POINT) {
        s.type = 0u; s.index = (uint)light_index;
        light_pdf = (1.0f / (float)light_count) * P.prob_point;
    } else if (kind == TRI) {
        s.type = 1u; s.index = (uint)light_index;
        const f3 A = F3(TR_F(L.r0.x), TR_F(L.r0.y), TR_F(L.r0.z)) - pos, B = F3(TR_F(L.r0.w), TR_F(L.r1.x), TR_F(L.r1.y)) - pos, C = F3(TR_F(L.r1.z), TR_F(L.r1.w), TR_F(L.r2.x)) - pos;
        float tri_pdf = 0.0f;
        const f3 out_dir = sample_triangle_light<RoundedMath>(1, F2(u.x, u.y), A, B, C, tri_pdf);
        const float out_length = ray_plane_intersection_dist(out_dir, A, B, C);
        if (isinf(tri_pdf) || tri_pdf <= 0 || out_length <= P.min_ray_dist || any_nan(out_dir)) tri_pdf = 1e9f;
        const f3 bary = get_barycentric_coords(out_dir * out_length, A, B, C);
        s.data = F2(bary.x, bary.y);
        light_pdf = (tri_pdf * (1.0f / (float)light_count)) * P.prob_tri;
    } else if (kind == DIR) {
        s.type = 2u; s.index = (uint)light_index;
        const float dir_cutoff = TR_F(L.r1.w);
        light_pdf = dir_cutoff >= 1.0f ? 1.0f : 1.0f / (2.0f * TR_PI * (1.0f - dir_cutoff));
        light_pdf = (light_pdf / (float)light_count) * P.prob_dir;
        s.data = F2(u.x, u.y);
    } else if (kind == ENV) {
        s.type = 3u; s.index = 0u;
        const uint sx = sv.env_w, sy = sv.env_h, pixel_count = sx * sy;
        int i = alias_i;
        light_pdf = TR_F(alias.z);
        if (rnd.z > alias.y) { i = (int)alias.x; light_pdf = TR_F(alias.w); }
        const int ppx = (int)((uint)i % sx), ppy = (int)((uint)i / sx);
        const f2 off = F2((float)(uint)(rnd.x * pixel_count), (float)(uint)(rnd.y * pixel_count)) * TR_INV_UINT32_MAX;
        s.data = (F2((float)ppx, (float)ppy) + off) / F2((float)sx, (float)sy);
        light_pdf = light_pdf * P.prob_env;
    }
#undef TR_F
    return s;
}

}  // namespace tr
