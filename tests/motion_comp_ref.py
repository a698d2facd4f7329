"""numpy restatement, in float64, of the front end's motion compensation (a helper, not a test module):

    MotionCompensation             builder/map_builder.cc:232-257
    common::InterpolateTransform   common/math.h:199-211
    common::AverageTransforms      common/math.cc:178-195
    Eigen::Quaternion(Matrix3), QuaternionBase::slerp, QuaternionBase::toRotationMatrix   Eigen/src/Geometry/Quaternion.h

Every product and sum is written in the order the reference evaluates it; nothing is fused.  Rows are InnerPointType rows
(x, y, z, intensity, factor) and come back as float32."""
import numpy as np

DBL_EPSILON = np.finfo(np.float64).eps


def quaternion_from_rotation(m):
    """Eigen's Quaternion(Matrix3) as (w, x, y, z): the trace branch, else the largest-diagonal branch (w may be negative)."""
    m = np.asarray(m, np.float64)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(3)
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return np.array([w, q[0], q[1], q[2]])


def slerp_plan(delta):
    """What q_a.slerp(t, q_b) derives from q_a = (1, 0, 0, 0) and q_b = Quaternion(delta's rotation) alone:
    dict(qb, d, linear, theta, sin_theta)."""
    qb = quaternion_from_rotation(np.asarray(delta, np.float64)[:3, :3])
    d = 0.0 * qb[1] + 0.0 * qb[2] + 0.0 * qb[3] + 1.0 * qb[0]                 # this->dot(other)
    abs_d = abs(d)
    linear = bool(abs_d >= 1.0 - DBL_EPSILON)
    theta = 0.0 if linear else float(np.arccos(abs_d))
    return dict(qb=qb, d=d, linear=linear, theta=theta, sin_theta=0.0 if linear else float(np.sin(theta)))


def slerp_scales(plan, t):
    t = np.asarray(t, np.float64)
    if plan["linear"]:
        s0, s1 = 1.0 - t, t.copy()
    else:
        s0 = np.sin((1.0 - t) * plan["theta"]) / plan["sin_theta"]
        s1 = np.sin(t * plan["theta"]) / plan["sin_theta"]
    if plan["d"] < 0:
        s1 = -s1
    return s0, s1


def interpolated_rotations(delta, factors):
    """q_a.slerp(f, q_b).toRotationMatrix() for every factor: [N, 3, 3] float64 (the quaternion is not normalised)."""
    plan = slerp_plan(delta)
    s0, s1 = slerp_scales(plan, np.asarray(factors, np.float32).astype(np.float64))
    w, x, y, z = plan["qb"]
    qx, qy, qz, qw = s0 * 0.0 + s1 * x, s0 * 0.0 + s1 * y, s0 * 0.0 + s1 * z, s0 * 1.0 + s1 * w
    tx, ty, tz = 2.0 * qx, 2.0 * qy, 2.0 * qz
    twx, twy, twz = tx * qw, ty * qw, tz * qw
    txx, txy, txz = tx * qx, ty * qx, tz * qx
    tyy, tyz, tzz = ty * qy, tz * qy, tz * qz
    R = np.empty((len(s0), 3, 3))
    R[:, 0, 0] = 1.0 - (tyy + tzz); R[:, 0, 1] = txy - twz; R[:, 0, 2] = txz + twy
    R[:, 1, 0] = txy + twz; R[:, 1, 1] = 1.0 - (txx + tzz); R[:, 1, 2] = tyz - twx
    R[:, 2, 0] = txz - twy; R[:, 2, 1] = tyz + twx; R[:, 2, 2] = 1.0 - (txx + tyy)
    return R


def interpolate_transform(delta, factor):
    """common::InterpolateTransform(I, delta, factor) as a 4x4."""
    if not (0.0 <= float(np.float32(factor)) <= 1.0):
        raise ValueError("CHECK(factor >= 0. && factor <= 1.)")
    delta = np.asarray(delta, np.float64)
    T = np.eye(4)
    T[:3, :3] = interpolated_rotations(delta, [factor])[0]
    T[:3, 3] = 0.0 + (delta[:3, 3] - 0.0) * float(np.float32(factor))
    return T


def motion_compensation_f64(rows5, delta):
    """The new points before the cast to float: [N, 3] float64."""
    rows = np.asarray(rows5, np.float32)
    delta = np.asarray(delta, np.float64)
    f32 = rows[:, 4]
    if not bool(np.all((f32 >= 0) & (f32 <= 1))):                                # NaN fails both comparisons
        raise ValueError("CHECK(factor >= 0. && factor <= 1.)")
    f = f32.astype(np.float64)
    R = interpolated_rotations(delta, f32)
    x, y, z = (rows[:, c].astype(np.float64) for c in range(3))
    out = np.empty((len(rows), 3))
    for r in range(3):
        out[:, r] = ((R[:, r, 0] * x + R[:, r, 1] * y) + R[:, r, 2] * z) + (0.0 + (delta[r, 3] - 0.0) * f)
    return out


def motion_compensation(rows5, delta):
    """MotionCompensation: [N, 5] float32 rows, intensity and factor carried over bit for bit."""
    rows = np.ascontiguousarray(np.asarray(rows5, np.float32))
    out = rows.copy()
    out[:, :3] = motion_compensation_f64(rows, delta).astype(np.float32)
    return out


def rotation_matrix_to_euler_angles(R):                                         # common/math.h:108-127
    sy = np.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0])
    if not sy < 1e-6:
        return np.array([np.arctan2(R[2, 1], R[2, 2]), np.arctan2(-R[2, 0], sy), np.arctan2(R[1, 0], R[0, 0])])
    return np.array([np.arctan2(-R[1, 2], R[1, 1]), np.arctan2(-R[2, 0], sy), 0.0])


def euler_angles_to_rotation_matrix(e):                                         # common/math.h:130-138: Rz * Ry * Rx
    cx, sx, cy, sy, cz, sz = np.cos(e[0]), np.sin(e[0]), np.cos(e[1]), np.sin(e[1]), np.cos(e[2]), np.sin(e[2])
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx],
                     [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]])


def average_transforms(transforms):
    """common::AverageTransforms: the mean translation and the mean of the x, y, z Euler angles."""
    assert len(transforms) > 0
    angles, translation = np.zeros(3), np.zeros(3)
    for T in transforms:
        T = np.asarray(T, np.float64)
        translation = translation + T[:3, 3]
        angles = angles + rotation_matrix_to_euler_angles(T[:3, :3])
    translation = translation / float(len(transforms))
    angles = angles / float(len(transforms))
    out = np.eye(4)
    out[:3, :3] = euler_angles_to_rotation_matrix(angles)
    out[:3, 3] = translation
    return out


def ulp_distance(a, b):
    """|a - b| in float32 units in the last place, elementwise (+0 and -0 are the same number); NaN anywhere gives a huge count."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)

    def ordered(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(ordered(a) - ordered(b))
    return np.where(np.isnan(a) | np.isnan(b), np.int64(1) << 40, d)


def assert_one_ulp(got, want, what=""):
    """The rule of the motion-compensation checks: every float coordinate within 1 ulp, at most 1e-4 of them different at all.
    Two correct double sin / acos differ by a few double ulps, i.e. ~1e-13 m in a coordinate; that changes the float only when
    the double lies that close to a rounding boundary, and then by exactly 1 ulp.  The cap keeps a wrong formula from hiding
    behind "1 ulp"."""
    d = ulp_distance(got, want)
    worst, differing = int(d.max()) if d.size else 0, int(np.count_nonzero(d))
    print("%s: max %d ulp, %d of %d coordinates differ" % (what, worst, differing, d.size))
    assert worst <= 1, (what, worst)
    assert differing <= 1e-4 * d.size, (what, differing, d.size)


def rotation_about(axis, angle):
    """Rodrigues' rotation matrix (test input, not part of the restatement)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1.0 - np.cos(angle)) * (K @ K)


def check_deltas():
    """The four deltas of the checks: a small drive motion, 3.1 rad about (-1, 0, 0) (q_b.w < 0 through the largest-diagonal
    branch), 1e-9 rad (the slerp's linear branch) and the identity."""
    def T(R, t):
        M = np.eye(4)
        M[:3, :3] = R
        M[:3, 3] = t
        return M
    drive = T(rotation_about((0.1, -0.2, 1.0), np.deg2rad(0.4)), (0.3, 0.01, -0.002))
    half_turn = T(rotation_about((-1.0, 0.0, 0.0), 3.1), (0.2, -0.1, 0.05))
    tiny = T(rotation_about((0.0, 0.0, 1.0), 1e-9), (0.3, 0.0, 0.0))
    return {"drive": drive, "half_turn": half_turn, "tiny": tiny, "identity": np.eye(4)}


