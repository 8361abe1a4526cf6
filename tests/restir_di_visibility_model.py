"""The visibility modes of ReSTIR DI (`visibility modes` of tauray_amd/csrc/restir_di.h) on top of
tests/restir_di_model.py.  The recorded visibilities make target = luminance(contribution * visibility) hold in every mode (point 1), so
the mode enters a frame in three places only: the neighbour pick (point 4), the multiply behind the candidates (point 2) and the multiply
ahead of the history store (point 6)."""
import numpy as np

import restir_di_model as M

PER_TARGET, SHARED, SAMPLED = 0, 1, 2
MODES = {"per-target": PER_TARGET, "shared": SHARED, "sampled": SAMPLED}


def untraced_visibility(contribution):
    """Point 1: the factor of a target that traces nothing - 1 where a shadow ray would be cast, 0 otherwise."""
    return (np.asarray(contribution) > 0).any(-1).astype(np.float32)


def pick_neighbours(px, py, offsets, size, surface_id, good_fn, spatial, mode):
    """M.pick_neighbours in mode 0; in modes 1 and 2 a bad neighbour takes no slot and the first `spatial` good ones are held in draw
    order.  Returns [(x, y, good)] per slot, (-1, -1, False) for an empty one."""
    if mode == PER_TARGET:
        return M.pick_neighbours(px, py, offsets, size, surface_id, good_fn, spatial)
    slots = [(-1, -1, False)] * spatial
    good = 0
    for ox, oy in offsets:
        x, y = px + int(ox), py + int(oy)
        if not (0 <= x < size[0] and 0 <= y < size[1]) or surface_id[y, x] < 0:
            continue
        if good_fn(x, y) and good < spatial:
            slots[good] = (x, y, True)
            good += 1
    return slots


def frame_slots(xs, ys, viewport, frame, options, size, surface, cam, mode, dt):
    """The spatial pass's neighbour slots of the pixels (xs, ys) of one viewport: the 2 * spatial_samples offset draws of the spatial
    stream, the good test against the downloaded surface records, the mode's pick.  (pixels, spatial_samples, 3) of (x, y, good)."""
    K = options["spatial_samples"]
    w, h = size
    s = surface[ys, xs]
    rs = M.init_sampler(xs, ys, viewport, 2 * frame + 1, options["rng_seed"])
    offs = []
    for _ in range(2 * K):
        rs = M.pcg4d(rs)
        offs.append(M.neighbour_offsets(M.unit(rs, dt)[:, :2], options["search_radius"], dt))
    offs = np.stack(offs, 1)
    inv = M.inv_max_plane_dist(cam["proj_inverse"], cam["view_inverse"], s["pos"], dt)
    nx, ny = xs[:, None] + offs[..., 0], ys[:, None] + offs[..., 1]
    on = (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
    ns = surface[np.where(on, ny, 0), np.where(on, nx, 0)]
    good = np.stack([M.neighbour_is_good(s, ns["pos"][:, k], ns["flat_normal"][:, k], inv, dt) for k in range(2 * K)], 1)
    sid = surface["instance_id"]
    slots = np.zeros((len(s), K, 3), dtype=np.int64)
    for p in range(len(s)):
        g = {(int(nx[p, k]), int(ny[p, k])): bool(good[p, k]) for k in range(2 * K) if on[p, k]}
        got = pick_neighbours(int(xs[p]), int(ys[p]), offs[p], size, sid, lambda x, y: g[(x, y)], K, mode)
        slots[p] = [(x, y, int(gd)) for x, y, gd in got]
    return slots


def model_frame(base_frame, run, scene, L, fi, v, dt, mode):
    """A frame of the model in `mode`.  base_frame: the frame model of mode 0 (test_restir_di._model_frame), which takes every visibility
    from the records and so serves every mode for the draws, the light picks and the continuous quantities; here the slots become the
    mode's pick.  Mode 2's two multiplies (sampled_multiply) are exact in float32 and belong to the replay of the records."""
    # base_frame also picks the slots by mode 0's rule, in its own per-pixel loop, and keeps neither its offsets nor its good bits:
    # frame_slots draws and tests them again.  The price of leaving tests/test_restir_di.py, where base_frame lives, byte for byte.
    out = base_frame(None, run, scene, L, fi, v, dt)
    f = run.frames[fi]
    ys, xs = out["ys"], out["xs"]
    if run.options["spatial_samples"]:
        cam = scene.camera_data()[run.viewports[v]]
        out["slots"] = frame_slots(xs, ys, run.viewports[v], fi, run.options, run.size, f["surface"][v], cam, mode, dt)
    return out


def sampled_multiply(uc_weight, visibility):
    """Points 2 and 6: uc_weight = uc_weight * visibility in float32."""
    return (np.asarray(uc_weight, dtype=np.float32) * np.asarray(visibility, dtype=np.float32)).astype(np.float32)


def ris_behind_a_half_plane(L, surface, hidden, candidates, mode, seed, dt):
    """RIS as the canonical kernel runs it over point lights at `surface` (n records), with an analytic occluder: hidden[i] says that
    light i is behind it.  Modes 1 and 2, no reuse.  Returns the estimate contribution * V * uc_weight (n, 3), the canonical uc_weight
    and the chosen light's index (NULL_INDEX: none)."""
    assert mode in (SHARED, SAMPLED)
    n = len(surface)
    hidden = np.asarray(hidden, dtype=bool)
    rs = M.init_sampler(np.arange(n) % 200, np.arange(n) // 200, 0, 0, seed)
    wsum, target, chosen = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt), np.full(n, M.NULL_INDEX)
    for _ in range(candidates):
        rs = M.pcg4d(rs)
        typ, idx, data, pdf = M.sample_canonical(L, rs, surface["pos"], 1e-4, dt)
        contrib = M.light_contribution(L, typ, idx, data, surface, dt)[0]
        t = M.luminance(contrib * untraced_visibility(contrib).astype(dt)[:, None], dt)      # point 1: no ray
        w = M.nan_to_zero((dt(1) / dt(candidates)) * t / pdf)
        rs = M.pcg4d(rs)
        wsum, take = M.update_reservoir(wsum, w, M.unit(rs, dt)[:, 0])
        chosen, target = np.where(take, idx, chosen), np.where(take, t, target)
    ucw = M.uc_weight(wsum, target, dt)
    contrib = M.light_contribution(L, np.zeros(n, dtype=int), chosen, np.zeros((n, 2)), surface, dt)[0]
    lit = chosen != M.NULL_INDEX
    V = np.where(lit & (contrib > 0).any(-1), ~hidden[np.where(lit, chosen, 0)], False).astype(dt)
    if mode == SAMPLED:
        ucw = ucw * V                        # point 2
    final = ucw * V if mode == SAMPLED else ucw      # point 6: once more ahead of the history store; V * V = V for an opaque occluder
    return (contrib * V[:, None]) * final[:, None], ucw, chosen
