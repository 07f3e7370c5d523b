"""SaveMap's files (xa.write_pcd / read_pcd, xa.write_tum, xa.write_g2o / read_g2o, xa.save_map) against the reference's
recorded run: trajectory.pcd, odom_tum.txt and pose_graph.g2o as pgo_node wrote them for its 1541 keyframes, kept whole
and byte for byte in tests/golden/pgo_run_1317618205/recorded.npz (one uint8 array per file).  The three files hold
the same poses (trajectory.pcd their positions as f32, the g2o file
position and quaternion at 6 significant digits, odom_tum.txt the camera-frame pose at 12), so each writer is checked
against its own recording: byte for byte where the recording carries its input at full precision, else within the input's
quantisation.  Host only.
"""
import os

import numpy as np
import pytest

from conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "pgo_run_1317618205", "recorded.npz")
N_KEYFRAMES = 1541


def gold_bytes(name) -> bytes:
    return np.load(GOLD)[name.replace(".", "_")].tobytes()


@pytest.fixture(scope="module")
def gold(tmp_path_factory):
    """The recorded files unpacked: name -> path."""
    d = tmp_path_factory.mktemp("pgo_run")
    for name in ("trajectory.pcd", "odom_tum.txt", "pose_graph.g2o"):
        (d / name).write_bytes(gold_bytes(name))
    return lambda name: str(d / name)


def quat_to_matrix(q):
    """Rotation matrix of a unit quaternion (x, y, z, w), as Eigen's toRotationMatrix."""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


@pytest.fixture(scope="module")
def vertices(gold):
    import xchu_slam_amd as xa
    v = xa.read_g2o(gold("pose_graph.g2o"))
    assert v.shape == (N_KEYFRAMES, 7)
    return v


def test_pcd_round_trip_is_byte_exact(tmp_path, gold):
    import xchu_slam_amd as xa
    cloud = xa.read_pcd(gold("trajectory.pcd"))
    assert cloud.shape == (N_KEYFRAMES, 4) and cloud.dtype == np.float32
    assert not cloud[:, 3].any()   # copyPointCloud of the key poses: intensity 0
    out = tmp_path / "trajectory.pcd"
    xa.write_pcd(out, cloud)
    assert out.read_bytes() == gold_bytes("trajectory.pcd")
    # an empty cloud is the eleven header lines alone
    xa.write_pcd(tmp_path / "empty.pcd", np.zeros((0, 4), np.float32))
    assert (tmp_path / "empty.pcd").read_text().splitlines()[-2:] == ["POINTS 0", "DATA ascii"]
    assert len((tmp_path / "empty.pcd").read_text().splitlines()) == 11
    assert xa.read_pcd(tmp_path / "empty.pcd").shape == (0, 4)


def test_g2o_round_trip_is_byte_exact(tmp_path, gold, vertices):
    import xchu_slam_amd as xa
    out = tmp_path / "pose_graph.g2o"
    xa.write_g2o(out, vertices)
    assert out.read_bytes() == gold_bytes("pose_graph.g2o")
    # the recording holds vertices only
    assert all(line.startswith("VERTEX_SE3:QUAT ") for line in open(gold("pose_graph.g2o")))


def test_tum_against_the_recording(tmp_path, gold, vertices):
    """write_tum of the g2o vertices' poses against the recorded odom_tum.txt.  Positions within 1e-3 m (the g2o input
    carries 6 significant digits of coordinates below 1000 m: up to 5e-4 each); quaternion components within 2e-6 with
    the recorded sign (input quantisation 5e-7 per component; an output component is half a signed sum of four input
    components, <= 1e-6, doubled for the normalisation).  Measured: 5.0e-4 and 4.98e-7, no sign flip."""
    import xchu_slam_amd as xa
    text = open(gold("odom_tum.txt")).read()
    rec = np.array([[float(v) for v in line.split()] for line in text.splitlines()])
    assert rec.shape == (N_KEYFRAMES, 8)
    # every recorded number re-formats to itself under %.12g
    assert "".join(" ".join("%.12g" % v for v in row) + "\n" for row in rec) == text
    M = np.tile(np.eye(4), (N_KEYFRAMES, 1, 1))
    for k, v in enumerate(vertices):
        M[k, :3, :3] = quat_to_matrix(v[3:] / np.linalg.norm(v[3:]))
        M[k, :3, 3] = v[:3]
    out = tmp_path / "odom_tum.txt"
    xa.write_tum(out, rec[:, 0], M)
    got_text = out.read_text()
    got = np.array([[float(v) for v in line.split()] for line in got_text.splitlines()])
    assert got.shape == rec.shape
    assert "".join(" ".join("%.12g" % v for v in row) + "\n" for row in got) == got_text
    assert np.array_equal(got[:, 0], rec[:, 0])
    pos_err = np.abs(got[:, 1:4] - rec[:, 1:4]).max()
    quat_err = np.abs(got[:, 4:] - rec[:, 4:]).max()   # no flip allowed: q and -q are 2 apart in some component
    print(f"odom_tum.txt: max position error {pos_err:.3e} m, max quaternion component error {quat_err:.3e}")
    assert pos_err <= 1e-3
    assert quat_err <= 2e-6


def test_tum_pose6d_path_matches_the_matrix_path(tmp_path):
    """Pose6D input goes through Pose6D2Matrix; the same poses as matrices give the same file within 1e-12.  Angles in
    every quadrant, so that the trace branch and each largest-diagonal branch of Eigen's conversion are taken."""
    import xchu_slam_amd as xa
    from xchu_slam_amd.globalmap import VELO2CAMERA, matrix_to_quaternion
    from xchu_slam_amd.synth import pose_matrix
    rng = np.random.default_rng(5)
    poses = np.concatenate([rng.uniform(-100, 100, (64, 3)), rng.uniform(-np.pi, np.pi, (64, 3))], 1)
    poses[0, 3:] = 0.0
    times = np.arange(64) * 0.1
    M = np.stack([pose_matrix(*p) for p in poses])
    xa.write_tum(tmp_path / "a.txt", times, poses)
    xa.write_tum(tmp_path / "b.txt", times, M)
    a = np.loadtxt(tmp_path / "a.txt")
    b = np.loadtxt(tmp_path / "b.txt")
    assert a.shape == (64, 8) and np.abs(a - b).max() <= 1e-12
    branches = set()
    for k, m in enumerate(M):
        R = (VELO2CAMERA @ m)[:3, :3]
        branches.add("trace" if np.trace(R) > 0 else int(np.argmax(np.diag(R))))
        q = np.array(matrix_to_quaternion(R))
        assert abs(np.linalg.norm(q) - 1.0) < 1e-12
        assert np.abs(quat_to_matrix(q) - R).max() < 1e-12   # the quaternion is the rotation's, whatever the branch
        assert np.abs(a[k, 4:] - q).max() <= 1e-11           # and what the file holds (12 digits)
        assert np.abs(a[k, 1:4] - (VELO2CAMERA @ m)[:3, 3]).max() <= 1e-9
    assert branches == {"trace", 0, 1, 2}
    # the identity lidar pose: the camera looks along the lidar's x, 0.08 m behind it
    assert np.abs(a[0, 4:] - np.array([0.5, -0.5, 0.5, 0.5])).max() < 1e-12
    assert np.abs(a[0, 1:4] - (VELO2CAMERA @ pose_matrix(*poses[0]))[:3, 3]).max() < 1e-9


def test_save_map_writes_the_five_files(tmp_path):
    """save_map with a ready map in place of the device store: each file reads back to what went in.  A PCD value is
    the f32 at 8 significant digits read back into f32: within 5e-8 (decimal) + 2^-24 (f32) of the value, relative."""
    import xchu_slam_amd as xa
    from xchu_slam_amd.globalmap import matrix_to_quaternion
    from xchu_slam_amd.synth import pose_matrix
    rng = np.random.default_rng(9)
    n = 7
    poses = np.concatenate([rng.uniform(-50, 50, (n, 3)), rng.uniform(-0.3, 0.3, (n, 3))], 1)
    times = np.arange(n) * 0.31
    cloud = np.concatenate([rng.uniform(-80, 80, (500, 3)), rng.uniform(0, 1, (500, 1))], 1).astype(np.float32)
    scans = np.concatenate([rng.uniform(-50, 50, (20, 3)), rng.uniform(-0.3, 0.3, (20, 3))], 1)
    stamps = np.arange(20) * 0.1
    d = tmp_path / "run"
    final = xa.save_map(d, cloud, poses, times, odom=(stamps, scans), leaf=0.5)
    assert sorted(os.listdir(d)) == ["finalMap.pcd", "lidar_odom.txt", "odom_tum.txt", "pose_graph.g2o", "trajectory.pcd"]
    assert np.array_equal(final, cloud)
    rel = 5e-8 + 2.0 ** -24
    back = xa.read_pcd(d / "finalMap.pcd")
    assert back.shape == cloud.shape and np.all(np.abs(back.astype(np.float64) - cloud) <= rel * np.abs(cloud))
    traj = xa.read_pcd(d / "trajectory.pcd")
    want = poses[:, :3].astype(np.float32)
    assert traj.shape == (n, 4) and not traj[:, 3].any()
    assert np.all(np.abs(traj[:, :3].astype(np.float64) - want) <= rel * np.abs(want))
    # writing what was read writes the same bytes
    xa.write_pcd(tmp_path / "again.pcd", xa.read_pcd(d / "finalMap.pcd"))
    assert (tmp_path / "again.pcd").read_bytes() == (d / "finalMap.pcd").read_bytes()
    for name, t, P in (("odom_tum.txt", times, poses), ("lidar_odom.txt", stamps, scans)):
        rows = np.loadtxt(d / name)
        assert rows.shape == (len(P), 8)
        for row, tk, p in zip(rows, t, P):
            cam = xa.globalmap.VELO2CAMERA @ pose_matrix(*p)
            ref = np.concatenate([[tk], cam[:3, 3], matrix_to_quaternion(cam[:3, :3])])
            assert np.all(np.abs(row - ref) <= 5e-12 * np.maximum(1.0, np.abs(ref)))   # 12 significant digits
    v = xa.read_g2o(d / "pose_graph.g2o")
    assert v.shape == (n, 7)
    for row, p in zip(v, poses):
        m = pose_matrix(*p)
        ref = np.concatenate([m[:3, 3], matrix_to_quaternion(m[:3, :3])])
        assert np.all(np.abs(row - ref) <= 5e-6 * np.maximum(1e-30, np.abs(ref)))      # %g: 6 significant digits
    # without odom there is no lidar_odom.txt
    xa.save_map(tmp_path / "run2", cloud, poses, times)
    assert sorted(os.listdir(tmp_path / "run2")) == ["finalMap.pcd", "odom_tum.txt", "pose_graph.g2o", "trajectory.pcd"]
