"""Host restatement of the sweep accumulator, written from the reference's two files and Eigen's
algorithms, not from the library's C++:

- VelodyneAccumulatorROS::processLidar / clearCloud / getCloud
  (aicp_ros/src/velodyne_accumulator.cpp:31-84): crop to the +-30 m cube in the sensor frame
  (getPointsInOrientedBox with the identity, i.e. pcl::CropBox: non-finite points removed, the
  bounds inclusive), pcl::transformPointCloud(cloud, offset, quaternion) in float, append, finished
  after batch_size sweeps, pushes ignored while finished.
- AppROS::velodyneCallBack's motion gate (aicp_ros/src/app_ros.cpp:203-213) in float64.
- Eigen 3.3: Quaternion(Matrix3) (QuaternionBase::operator=(MatrixBase), the trace /
  largest-diagonal branches), Quaternion::toRotationMatrix (no normalisation), and an Isometry's
  rotation() taken as its linear part as it stands.

Every float step rounds to float32 on its own (separate multiply and add, no FMA).

Neither PCL nor Eigen is installed where these tests run, so parity with them is NOT pinned here,
as for the crop and the pre-filter: which Eigen version stands behind rotation() (later versions
extract the rotation by an SVD for a general Transform; for an Isometry all of them take the linear
part), and that PCL 1.8's transformPointCloud evaluates the plain float expression
r00 x + r01 y + r02 z + t0 left to right, are read from their sources, not measured.
"""
import numpy as np

F = np.float32


def quat_from_matrix(m, S):
    """Eigen::Quaternion<S>(Matrix3): (x, y, z, w), every step in S."""
    m = np.asarray(m, S)
    one, half = S(1), S(0.5)
    q = [S(0)] * 4
    t = S(S(m[0, 0] + m[1, 1]) + m[2, 2])
    if t > S(0):
        t = S(np.sqrt(S(t + one)))
        q[3] = S(half * t)
        t = S(half / t)
        q[0] = S(S(m[2, 1] - m[1, 2]) * t)
        q[1] = S(S(m[0, 2] - m[2, 0]) * t)
        q[2] = S(S(m[1, 0] - m[0, 1]) * t)
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = S(np.sqrt(S(S(S(m[i, i] - m[j, j]) - m[k, k]) + one)))
        q[i] = S(half * t)
        t = S(half / t)
        q[3] = S(S(m[k, j] - m[j, k]) * t)
        q[j] = S(S(m[j, i] + m[i, j]) * t)
        q[k] = S(S(m[k, i] + m[i, k]) * t)
    return q


def quat_branch(m):
    """Which of Eigen's four branches a rotation block takes: 'trace', or the largest diagonal 0 / 1 / 2."""
    m = np.asarray(m, F)
    if F(F(m[0, 0] + m[1, 1]) + m[2, 2]) > F(0):
        return "trace"
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    return i


def matrix_from_quat(q, S):
    """Eigen::Quaternion<S>::toRotationMatrix, every step in S."""
    x, y, z, w = (S(v) for v in q)
    two, one = S(2), S(1)
    tx, ty, tz = S(two * x), S(two * y), S(two * z)
    twx, twy, twz = S(tx * w), S(ty * w), S(tz * w)
    txx, txy, txz = S(tx * x), S(ty * x), S(tz * x)
    tyy, tyz, tzz = S(ty * y), S(tz * y), S(tz * z)
    return np.array([[S(one - S(tyy + tzz)), S(txy - twz), S(txz + twy)],
                     [S(txy + twz), S(one - S(txx + tzz)), S(tyz - twx)],
                     [S(txz - twy), S(tyz + twx), S(one - S(txx + tyy))]], S)


def pose_matrix(pose):
    """The sweep's float 4x4 (row-major numpy) from its Isometry3d `pose` (4x4 float64, row-major):
    Translation3f(pose.translation().cast<float>()) * Quaternionf(pose.rotation().cast<float>())."""
    P = np.asarray(pose, np.float64).reshape(4, 4)
    T = np.eye(4, dtype=F)
    T[:3, :3] = matrix_from_quat(quat_from_matrix(P[:3, :3].astype(F), F), F)
    T[:3, 3] = P[:3, 3].astype(F)
    return T


def keep_mask(pts, mn=-30.0, mx=30.0):
    """pcl::CropBox with the identity frame: finite, and inside the closed cube."""
    p = np.asarray(pts, F)[:, :3]
    with np.errstate(invalid="ignore"):
        return np.isfinite(p).all(axis=1) & (p >= F(mn)).all(axis=1) & (p <= F(mx)).all(axis=1)


def transform(pts, T):
    """pcl::transformPointCloud in float32: ((r00 x + r01 y) + r02 z) + t0, each step rounded."""
    p = np.asarray(pts, F)[:, :3]
    T = np.asarray(T, F)
    out = np.empty((p.shape[0], 3), F)
    for r in range(3):
        s = (T[r, 0] * p[:, 0]).astype(F)
        s = (s + (T[r, 1] * p[:, 1]).astype(F)).astype(F)
        s = (s + (T[r, 2] * p[:, 2]).astype(F)).astype(F)
        out[:, r] = (s + T[r, 3]).astype(F)
    return out


class Accumulator:
    """VelodyneAccumulatorROS's state machine on numpy arrays."""

    def __init__(self, batch_size=80, crop_min=-30.0, crop_max=30.0):
        self.batch_size, self.crop_min, self.crop_max = int(batch_size), crop_min, crop_max
        self.clear()

    def clear(self):
        self.cloud = np.zeros((0, 3), F)
        self.kept = []
        self.counter = 0
        self.finished = False

    def push(self, pts, pose):
        if self.finished:
            return
        p = np.asarray(pts, F)
        p = p[:, :3] if p.size else np.zeros((0, 3), F)
        p = p[keep_mask(p, self.crop_min, self.crop_max)]
        self.cloud = np.concatenate([self.cloud, transform(p, pose_matrix(pose))], axis=0)
        self.kept.append(len(p))
        self.counter += 1
        if self.counter >= self.batch_size:
            self.finished = True

    def kept_per_sweep(self):
        out = np.zeros(self.batch_size, np.uint32)
        out[:len(self.kept)] = self.kept
        return out


def general_pose(yaw_deg=37.0, pitch_deg=-8.0, roll_deg=5.0, t=(12.5, -7.25, 0.8)):
    """A general Isometry3d (4x4 float64, row-major)."""
    from aicp_mapping_amd import synthetic as sy

    return sy.make_T(yaw_deg, pitch_deg, roll_deg, t)


def bridge_sweeps(seed=7):
    """The bridge tests' input: 3 sweeps of one small synthetic scene, each in its own sensor frame
    (the world points moved by the inverse of the sweep's pose), and the 3 poses. Accumulated, they
    give a raw cloud on which the pre-filter finds planes (tests/test_accumulator_cpu.py pins that)."""
    from aicp_mapping_amd import synthetic as sy

    scene = sy.make_scene(seed)
    sweeps, poses = [], []
    for i, (yaw, x) in enumerate([(3.0, -0.6), (-5.0, 0.0), (8.0, 0.7)]):
        P = sy.make_T(yaw, 0.5 * i, -0.4 * i, (x, 0.1 * i, 0.7))
        world = sy.sample_scene(scene, np.random.default_rng(seed + 1 + i), (x, 0.0, 0.7), half=3.0, spacing=0.05)
        sweeps.append(sy.transform(np.linalg.inv(P), world))
        poses.append(P)
    return sweeps, poses


def quat_to_euler(q):
    """common.cpp:70-78 on (x, y, z, w), float64."""
    q1, q2, q3, q0 = (float(v) for v in q)
    roll = np.arctan2(2 * (q0 * q1 + q2 * q3), 1 - 2 * (q1 * q1 + q2 * q2))
    pitch = np.arcsin(2 * (q0 * q2 - q3 * q1))
    yaw = np.arctan2(2 * (q0 * q3 + q1 * q2), 1 - 2 * (q2 * q2 + q3 * q3))
    return roll, pitch, yaw


def relative_motion(prev, pose):
    """prev.inverse() * pose for two Isometry3d (the Isometry inverse: R^T, -R^T t), sums left to
    right in float64. Returns (rotation 3x3, translation 3)."""
    A = np.asarray(prev, np.float64).reshape(4, 4)
    B = np.asarray(pose, np.float64).reshape(4, 4)
    Ri = A[:3, :3].T
    ti = np.array([-((Ri[r, 0] * A[0, 3] + Ri[r, 1] * A[1, 3]) + Ri[r, 2] * A[2, 3]) for r in range(3)])
    R = np.array([[(Ri[r, 0] * B[0, c] + Ri[r, 1] * B[1, c]) + Ri[r, 2] * B[2, c] for c in range(3)]
                  for r in range(3)])
    t = np.array([((Ri[r, 0] * B[0, 3] + Ri[r, 1] * B[1, 3]) + Ri[r, 2] * B[2, 3]) + ti[r] for r in range(3)])
    return R, t


def motion_terms(prev, pose):
    """(distance, roll, pitch, yaw) of the relative motion, as velodyneCallBack computes them."""
    R, t = relative_motion(prev, pose)
    dist = float(np.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]))
    return (dist,) + tuple(float(a) for a in quat_to_euler(quat_from_matrix(R, np.float64)))


def motion_gate(prev, pose, min_dist=1.0, min_angle=10.0 * np.pi / 180.0):
    d, r, p, y = motion_terms(prev, pose)
    return bool(d > min_dist or abs(r) > min_angle or abs(p) > min_angle or abs(y) > min_angle)
