"""numpy model of tauray_amd/csrc/morph.h: the order of operations of k_morph, operation by operation, at float32 (every product, sum,
square root and quotient a correctly rounded float32 operation, as numpy's are) or at float64 (the yardstick of the float32 model's own
rounding).  Vertices are tauray_amd.scene.VERTEX records; planes are (T, V, 3) arrays or None."""
import numpy as np


def active_list(weights):
    """The (index, weight) pairs of the non-zero weights, ascending: what the host compacts for the kernel."""
    w = np.asarray(weights, dtype=np.float32)
    return [(k, w[k]) for k in range(len(w)) if w[k] != 0]


def _accumulate(base, plane, active, dtype):
    acc = base.astype(dtype)
    for k, w in active:
        acc = acc + dtype(w) * plane[k].astype(dtype)      # one rounding for the product, one for the sum
    return acc


def _direction(acc, base, dtype):
    d = (acc[:, 0] * acc[:, 0] + acc[:, 1] * acc[:, 1]) + acc[:, 2] * acc[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        length = np.sqrt(d)
        out = acc / length[:, None]
    keep = ~(length > 0)
    out[keep] = base.astype(dtype)[keep]
    return out


def morph(vertices, weights, dpos, dnrm=None, dtan=None, dtype=np.float32):
    """The morphed vertices.  dtype float32: VERTEX records with the kernel's bits.  dtype float64: a dict of float64 arrays
    (pos, normal, tangent), the same formulas without float32 rounding."""
    active = active_list(weights)
    if dtype == np.float32:
        out = vertices.copy()
        if not active:
            return out
        out["pos"] = _accumulate(vertices["pos"], dpos, active, np.float32)
        if dnrm is not None:
            out["normal"] = _direction(_accumulate(vertices["normal"], dnrm, active, np.float32), vertices["normal"], np.float32)
        if dtan is not None:
            out["tangent"][:, :3] = _direction(_accumulate(vertices["tangent"][:, :3], dtan, active, np.float32), vertices["tangent"][:, :3], np.float32)
        return out
    out = dict(pos=vertices["pos"].astype(np.float64), normal=vertices["normal"].astype(np.float64), tangent=vertices["tangent"].astype(np.float64))
    if not active:
        return out
    out["pos"] = _accumulate(vertices["pos"], dpos, active, np.float64)
    if dnrm is not None:
        out["normal"] = _direction(_accumulate(vertices["normal"], dnrm, active, np.float64), vertices["normal"], np.float64)
    if dtan is not None:
        out["tangent"][:, :3] = _direction(_accumulate(vertices["tangent"][:, :3], dtan, active, np.float64), vertices["tangent"][:, :3], np.float64)
    return out


def random_mesh(seed, vertex_count, target_count, normals=True, tangents=True):
    """A seeded mesh for the tests: unit normals and tangents, positions in [-1, 1], deltas of a few tenths."""
    from tauray_amd.scene import VERTEX
    rng = np.random.default_rng(seed)
    v = np.zeros(vertex_count, dtype=VERTEX)
    v["pos"] = rng.uniform(-1, 1, (vertex_count, 3))
    for name, n in (("normal", 3), ("tangent", 3)):
        d = rng.normal(size=(vertex_count, 3))
        v[name][:, :3] = d / np.linalg.norm(d, axis=1, keepdims=True)
    v["tangent"][:, 3] = rng.choice([-1.0, 1.0], vertex_count)
    v["uv"] = rng.uniform(0, 1, (vertex_count, 2))
    plane = lambda: rng.uniform(-0.3, 0.3, (target_count, vertex_count, 3)).astype(np.float32)
    return v, plane(), (plane() if normals else None), (plane() if tangents else None)
