"""A float64 brute-force ray / triangle reference and the closed meshes and aimed ray families of tests/test_watertight.py.

Numpy only; nothing here comes from oracle/ or from the library.  The intersector is Moeller-Trumbore over every triangle - another
formula than the watertight test of csrc/trace.h and oracle/oracle.cc, no tree, no slab test, no padding - so a mistake those two share
is not shared here.  The float32 numbers (rays as given to trace_closest, vertices as the device holds them) are the geometry: they
are promoted to float64 as they stand."""
import numpy as np

N_RAYS = 4096
BARY_EPS = 1e-12        # a triangle counts when min(u, v, 1 - u - v) >= -BARY_EPS


# ---------------------------------------------------------------------------------------------------------------------------------
# the intersector

def brute_force(rays, P, tri, chunk=256):
    """rays: (n, 8) float32 (origin, tmin, direction, tmax); P: (nv, 3) world-space vertices; tri: (nt, 3) indices.
    Returns (T, I, margin) per ray: the nearest distance (inf for none), its triangle (-1) and that triangle's min(u, v, 1 - u - v)."""
    rays = np.asarray(rays).astype(np.float64).reshape(-1, 8)
    P = np.asarray(P).astype(np.float64)
    tri = np.asarray(tri).reshape(-1, 3)
    v0, e1, e2 = P[tri[:, 0]], P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]]
    n = len(rays)
    T, I, M = np.full(n, np.inf), np.full(n, -1, np.int64), np.full(n, np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for lo in range(0, n, chunk):
            r = rays[lo:lo + chunk]
            o, d, tmin, tmax = r[:, None, 0:3], r[:, None, 4:7], r[:, None, 3], r[:, None, 7]
            p = np.cross(d, e2[None])
            det = (e1[None] * p).sum(-1)
            s = o - v0[None]
            u = (s * p).sum(-1) / det
            q = np.cross(s, e1[None])
            v = (d * q).sum(-1) / det
            t = (e2[None] * q).sum(-1) / det
            m = np.minimum(np.minimum(u, v), 1.0 - u - v)
            ok = (det != 0) & (m >= -BARY_EPS) & (t > tmin) & (t < tmax)      # NaN compares false
            t = np.where(ok, t, np.inf)
            i = t.argmin(1)
            k = np.arange(len(r))
            hit = ok[k, i]
            T[lo:lo + chunk] = t[k, i]
            I[lo:lo + chunk] = np.where(hit, i, -1)
            M[lo:lo + chunk] = np.where(hit, m[k, i], np.nan)
    return T, I, M


def shares_vertex(tri, a, b):
    """Per ray: do triangles a[i] and b[i] have a vertex in common (a triangle shares its vertices with itself; -1 shares none)?"""
    tri = np.asarray(tri).reshape(-1, 3)
    a, b = np.asarray(a), np.asarray(b)
    ok = (a >= 0) & (b >= 0)
    ta, tb = tri[np.where(ok, a, 0)], tri[np.where(ok, b, 0)]
    return ok & (ta[:, :, None] == tb[:, None, :]).any((1, 2))


def hit_points(P, tri, prim, u, v):
    """The point of triangle `prim` at weights (1 - u - v, u, v), in float64."""
    P = np.asarray(P).astype(np.float64)
    c = np.asarray(tri).reshape(-1, 3)[np.asarray(prim)]
    u, v = np.asarray(u).astype(np.float64)[:, None], np.asarray(v).astype(np.float64)[:, None]
    return (1.0 - u - v) * P[c[:, 0]] + u * P[c[:, 1]] + v * P[c[:, 2]]


# ---------------------------------------------------------------------------------------------------------------------------------
# meshes: (float32 vertices, int32 triangles), indexed, vertices shared

def icosphere(level):
    """The unit icosahedron, every triangle split in four `level` times, vertices on the unit sphere: 10 * 4^level + 2 vertices."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    verts = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in verts]
    tris = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
            (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(level):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in tris:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tris = out
    return np.asarray(verts).astype(np.float32), np.asarray(tris, np.int32)


def bipyramid(n):
    """A ring of n vertices at radius 1 in z = 0 (0 .. n - 1), apexes at z = +1 (n) and z = -1 (n + 1): 2 n needle triangles."""
    a = 2.0 * np.pi * np.arange(n) / n
    verts = np.concatenate([np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1), [(0, 0, 1), (0, 0, -1)]]).astype(np.float32)
    k, k1 = np.arange(n), (np.arange(n) + 1) % n
    tris = np.concatenate([np.stack([k, k1, np.full(n, n)], 1), np.stack([k1, k, np.full(n, n + 1)], 1)])
    return verts, tris.astype(np.int32)


def lattice(n, heights):
    """(n + 1)^2 vertices at spacing 2 / n on [-1, 1]^2, z = heights[row, column]; vertex j * (n + 1) + i is column i of row j, and cell
    (i, j) with corners a, b = a + 1, c = a + n + 1, d = c + 1 is split along a - d into (a, b, d) and (a, d, c), as scenes._grid_mesh does."""
    g = -1.0 + 2.0 * np.arange(n + 1) / n
    xx, yy = np.meshgrid(g, g, indexing="xy")
    verts = np.stack([xx.ravel(), yy.ravel(), np.asarray(heights, np.float64).reshape(n + 1, n + 1).ravel()], 1).astype(np.float32)
    i = np.arange(n)[None, :] + (n + 1) * np.arange(n)[:, None]
    a, b, c, d = i, i + 1, i + n + 1, i + n + 2
    return verts, np.stack([a, b, d, a, d, c], -1).reshape(-1, 3).astype(np.int32)


def bumpy_heights(n, seed):
    """Random multiples of 1/16 in [-0.5, 0.5] for lattice(n, .)."""
    return np.random.default_rng(seed).integers(-8, 9, size=(n + 1, n + 1)) / 16.0


def world_vertices(scene):
    """float32 world positions of every instance's vertices in the device's order, ((m[r,0] x + m[r,1] y) + m[r,2] z) + m[r,3], and the
    triangles over them (instance after instance), as tests/test_accel_strategies.py::_identity_scene computes them."""
    verts, tris, base = [], [], 0
    for i in range(len(scene.instances)):
        sp = scene.spans[i]
        p = scene.vertices["pos"][sp["vertex_offset"]:sp["vertex_offset"] + sp["vertex_count"]].astype(np.float32)
        m = np.asarray(scene.instances["model"][i], np.float32).T        # stored column-major
        w = np.empty_like(p)
        for r in range(3):
            w[:, r] = ((m[r, 0] * p[:, 0] + m[r, 1] * p[:, 1]) + m[r, 2] * p[:, 2]) + m[r, 3]
        assert w.dtype == np.float32
        verts.append(w)
        tris.append(np.asarray(scene.indices[sp["index_offset"]:sp["index_offset"] + 3 * sp["triangle_count"]], np.int64).reshape(-1, 3) + base)
        base += len(w)
    return np.concatenate(verts), np.concatenate(tris).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# ray families.  Everything is drawn and decided in float64; the rays are rounded to float32 once, at the end.

def _edges(tri):
    """Unique undirected edges (ne, 2) and, per edge, its two triangles (ne, 2) (-1 for a boundary edge's missing one)."""
    tri = np.asarray(tri).reshape(-1, 3)
    e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), 1)
    owner = np.tile(np.arange(len(tri)), 3)
    uniq, inv = np.unique(e, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    adj = np.full((len(uniq), 2), -1, np.int64)
    for k in np.argsort(inv, kind="stable"):
        slot = 0 if adj[inv[k], 0] < 0 else 1
        adj[inv[k], slot] = owner[k]
    return uniq, adj


def _vertex_triangles(tri, nv):
    """Per vertex the triangles around it, padded with -1 to the largest valence."""
    tri = np.asarray(tri).reshape(-1, 3)
    lists = [[] for _ in range(nv)]
    for t, c in enumerate(tri):
        for v in c:
            lists[v].append(t)
    out = np.full((nv, max(len(x) for x in lists)), -1, np.int64)
    for v, x in enumerate(lists):
        out[v, :len(x)] = x
    return out


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _pack(org, d, tmin):
    n = len(org)
    return np.concatenate([org, np.full((n, 1), tmin), d, np.full((n, 1), np.inf)], 1).astype(np.float32)


def _extent(P):
    P = np.asarray(P, np.float64)
    return P.mean(0), (P.max(0) - P.min(0)) / 2.0


def _targets(kind, P, tri, rng, n, inside):
    """n targets: the first half (inside: of the aimed rays) vertices, the second half points on edges.  Returns (points, adjacency
    rows padded with -1).  The bipyramid takes an apex for half of its vertex targets and, from the inside, its spokes for the edges."""
    nv = len(P)
    vt = _vertex_triangles(tri, nv)
    edges, et = _edges(tri)
    nvert = n // 2
    v = rng.integers(0, nv, nvert)
    if kind == "bipyramid":
        apex = rng.random(nvert) < 0.5
        v = np.where(apex, nv - 2 + rng.integers(0, 2, nvert), rng.integers(0, nv - 2, nvert))
        if inside:
            spoke = (edges >= nv - 2).any(1)
            edges, et = edges[spoke], et[spoke]
    e = rng.integers(0, len(edges), n - nvert)
    s = rng.random(n - nvert)[:, None]
    pts = np.concatenate([P[v], (1.0 - s) * P[edges[e, 0]] + s * P[edges[e, 1]]])
    adj = np.full((n, vt.shape[1]), -1, np.int64)
    adj[:nvert] = vt[v]
    adj[nvert:, :2] = et[e]
    return pts, adj


def inside(kind, P, tri, seed, tmin, n=N_RAYS):
    """Origins uniform in a ball around the centroid (radius 0.3 of the smallest half-extent; 0.2 for the bipyramid); a third of the
    rays at vertices, a third at points on edges, a third in uniform directions.  Returns (rays, adjacency): the triangles around each
    ray's target, rows padded with -1 (all -1 for the unaimed third)."""
    P = np.asarray(P).astype(np.float64)
    rng = np.random.default_rng(seed)
    c, half = _extent(P)
    radius = (0.2 if kind == "bipyramid" else 0.3) * half.min()
    org = c + _unit(rng, n) * (radius * rng.random(n) ** (1.0 / 3.0))[:, None]
    aimed = 2 * (n // 3)
    pts, adj_t = _targets(kind, P, tri, rng, aimed, True)
    d = np.concatenate([pts - org[:aimed], _unit(rng, n - aimed)])
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    adj = np.full((n, adj_t.shape[1]), -1, np.int64)
    adj[:aimed] = adj_t
    return _pack(org, d, tmin), adj


def outside(kind, P, tri, seed, tmin, n=N_RAYS):
    """Origins on the sphere of radius 3 x the largest half-extent around the centroid (3 for the unit meshes), aimed at vertices and
    points on edges all of whose triangles face the origin with cos > 0.3: a target is redrawn, origin and all, until they do.
    Silhouettes, which float32 cannot decide, are excluded by that."""
    P = np.asarray(P).astype(np.float64)
    tri = np.asarray(tri).reshape(-1, 3)
    rng = np.random.default_rng(seed)
    c, half = _extent(P)
    nrm = np.cross(P[tri[:, 1]] - P[tri[:, 0]], P[tri[:, 2]] - P[tri[:, 0]])
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= np.sign((nrm * (P[tri].mean(1) - c)).sum(1))[:, None]        # outward: the meshes are convex around their centroid
    org, pts, adj = np.zeros((n, 3)), np.zeros((n, 3)), None
    todo = np.arange(n)
    for _ in range(1000):
        if not len(todo):
            break
        # vertex and edge targets alternate by ray index, so that a redraw keeps the ray's kind
        p, a = _targets(kind, P, tri, rng, 2 * len(todo), False)
        is_edge = (todo % 2).astype(bool)
        p = np.where(is_edge[:, None], p[len(todo):], p[:len(todo)])
        a = np.where(is_edge[:, None], a[len(todo):], a[:len(todo)])
        o = c + _unit(rng, len(todo)) * (3.0 * half.max())
        to = o - p
        to /= np.linalg.norm(to, axis=1, keepdims=True)
        cos = (nrm[np.maximum(a, 0)] * to[:, None, :]).sum(-1)
        ok = np.where(a >= 0, cos, 1.0).min(1) > 0.3
        if adj is None:
            adj = np.full((n, a.shape[1]), -1, np.int64)
        org[todo[ok]], pts[todo[ok]], adj[todo[ok]] = o[ok], p[ok], a[ok]
        todo = todo[~ok]
    assert not len(todo), f"{len(todo)} rays found no target that faces them"
    d = pts - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _pack(org, d, tmin), adj


def exact(P, tri, n, tmin, tilt_seed=None, z0=8.0):
    """Lattice meshes (lattice(n, .) under a dyadic placement): from z = z0 at every interior vertex, the midpoint of the axis edge to
    its +x and to its +y neighbour, and the midpoint of its cell's diagonal - 4 (n - 1)^2 rays.  Direction (0, 0, -1); with `tilt_seed`
    (flat lattice) the unnormalised (i/64, j/64, -1), i, j in [-4, 4] drawn per ray, from an origin moved back so that the target
    stays where it is.  Every number is dyadic, float32 holds the rays exactly (asserted), and so every edge function that should be
    zero is zero in float32.  Returns (rays, adjacency)."""
    P = np.asarray(P).astype(np.float64)
    tri = np.asarray(tri).reshape(-1, 3)
    jj, ii = np.meshgrid(np.arange(1, n), np.arange(1, n), indexing="ij")
    a = (jj * (n + 1) + ii).ravel()
    vt = _vertex_triangles(tri, len(P))
    cell = 2 * ((a // (n + 1)) * n + a % (n + 1))                       # first triangle of the cell whose corner a is
    below, left = cell - 2 * n, cell - 2
    pts = np.concatenate([P[a], (P[a] + P[a + 1]) / 2, (P[a] + P[a + n + 1]) / 2, (P[a] + P[a + n + 2]) / 2])
    m = len(a)
    adj = np.full((4 * m, vt.shape[1]), -1, np.int64)
    adj[:m] = vt[a]
    adj[m:2 * m, :2] = np.stack([cell, below + 1], 1)                   # edge a - b: (a, b, d) of this cell, (a, d, c) of the one below
    adj[2 * m:3 * m, :2] = np.stack([cell + 1, left], 1)                # edge a - c: (a, d, c) of this cell, (a, b, d) of the one to the left
    adj[3 * m:, :2] = np.stack([cell, cell + 1], 1)
    for k, step in ((1, 1), (2, n + 1), (3, n + 2)):                    # the adjacency is what it says: both triangles hold the edge
        for t in adj[k * m:(k + 1) * m, :2].T:
            assert ((tri[t] == a[:, None]).any(1) & (tri[t] == (a + step)[:, None]).any(1)).all()
    d = np.tile([0.0, 0.0, -1.0], (4 * m, 1))
    org = np.concatenate([pts[:, :2], np.full((4 * m, 1), z0)], 1)
    if tilt_seed is not None:
        assert (pts[:, 2] == pts[0, 2]).all(), "tilted rays need the flat lattice"
        ij = np.random.default_rng(tilt_seed).integers(-4, 5, size=(4 * m, 2)) / 64.0
        d[:, :2] = ij
        org[:, :2] -= (z0 - pts[0, 2]) * ij
    rays64 = np.concatenate([org, np.full((4 * m, 1), tmin), d, np.full((4 * m, 1), np.inf)], 1)
    rays = rays64.astype(np.float32)
    assert (rays[:, [0, 1, 2, 4, 5, 6]].astype(np.float64) == rays64[:, [0, 1, 2, 4, 5, 6]]).all(), "float32 does not hold these rays"
    return rays, adj
