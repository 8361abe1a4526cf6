"""The rule of trhip_scene_set_deformation_motion (tauray_amd/csrc/shading.h surface_prev_pos) in numpy.

The previous world position of a hit with barycentrics (u, v) on triangle (i0, i1, i2) of an instance is

    model_prev * (P[i0] * (1 - u - v) + P[i1] * u + P[i2] * v, 1)

where P holds the model-space positions of the mesh as the last latch found them (switch on) or as they are now (switch off: the
reference's CALC_PREV_VERTEX_POS, shader/rt.glsl:73-79).  `previous_world_position` evaluates it in the kernel's order of operations at the
requested precision: every product and sum rounded on its own (the build has contraction off), the matrix product as common.h `mul` does it
(column 0 * x + column 1 * y + column 2 * z + column 3 * w, left to right).

Where the deformation from the previous to the current pose is one affine map A of the whole mesh (previous = A * current), interpolation
commutes with it and the same position is (model_prev * A) * interp(current): `affine_expected` - what an unchanged oracle computes from
the current vertices as a static mesh.  A is formed in float64 and rounded once."""
import numpy as np

f32 = np.float32


def interpolate(positions, triangle, u, v, dtype=f32):
    p = np.asarray(positions).astype(dtype)
    u, v = dtype(u), dtype(v)
    b = (dtype(1.0) - u - v, u, v)
    i0, i1, i2 = (int(x) for x in triangle)
    return p[i0] * b[0] + p[i1] * b[1] + p[i2] * b[2]


def transform_point(m, p, dtype=f32):
    """common.h mul(m, (p, 1)).xyz with m a 4 x 4 matrix as numpy writes it (row-major)."""
    m = np.asarray(m).astype(dtype)
    p = np.asarray(p).astype(dtype)
    return (((m[:3, 0] * p[0] + m[:3, 1] * p[1]) + m[:3, 2] * p[2]) + m[:3, 3] * dtype(1.0)).astype(dtype)


def previous_world_position(model_prev, previous_positions, triangle, u, v, dtype=f32):
    return transform_point(model_prev, interpolate(previous_positions, triangle, u, v, dtype), dtype)


def affine_between(pose_previous, pose_current):
    """A with previous = A * current for a mesh every vertex of which is pose * rest: A = pose_previous * inverse(pose_current), in float64."""
    return np.asarray(pose_previous, np.float64) @ np.linalg.inv(np.asarray(pose_current, np.float64))


def affine_expected(model_prev, A, current_positions, triangle, u, v, dtype=f32):
    """(model_prev * A) * interp(current): the matrix formed in float64 and rounded to float32 once, as an instance record holds it."""
    m = (np.asarray(model_prev, np.float64) @ np.asarray(A, np.float64)).astype(f32)
    return transform_point(m, interpolate(current_positions, triangle, u, v, dtype), dtype)


def rigid(rotation_quarter_turns_z=0, translation=(0.0, 0.0, 0.0), quarter_turns_x=0):
    """Rotation by whole quarter turns (entries 0 and +-1) and a translation: with translations that are multiples of 1/8 every product of
    such matrices, and their action on coordinates that are small multiples of a power of two, is exact in float32."""
    def rot(k, axis):
        c, s = [(1, 0), (0, 1), (-1, 0), (0, -1)][k % 4]
        r = np.eye(4)
        a, b = [(1, 2), (0, 2), (0, 1)][axis]
        r[a, a], r[a, b], r[b, a], r[b, b] = c, -s, s, c
        return r
    m = rot(rotation_quarter_turns_z, 2) @ rot(quarter_turns_x, 0)
    m[:3, 3] = translation
    return m
