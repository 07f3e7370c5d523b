"""The keyframe store and the global map on the device (xa.KeyframeMap, ndt_map_*; refine_loop / close_loops with a
store), bit for bit against what the parent library already computes: a stacked selection equals the concatenation of
icp_restate.transform_f32 (and of per-keyframe ndt_transform_device), a map equals pcl::VoxelGrid of that stack as
xa.voxel_downsample and the CPU restatement compute it, and loop closure from a store equals loop closure from host
keyframes.

Keyframe sizes are drawn around the points P one k_map_stack workgroup takes at a time (read from ndt_map_geometry): 0, 1,
P - 1, P, P + 1, 2 P + 1, with empty keyframes first, last and next to each other.
"""
import ctypes as C

import numpy as np
import pytest

import icp_restate as R
import oracle_lib

pytestmark = pytest.mark.gpu

xa = pytest.importorskip("xchu_slam_amd")
from xchu_slam_amd import _lib  # noqa: E402


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(bits(a), bits(b))


def last_error(store):
    return store._lib.ndt_last_error(store.ctx).decode()


class DeviceBuffer:
    """A device buffer of float4 points on a store's context."""

    def __init__(self, store, points):
        self.reg, self.points, self.ptr = store.registration, points, C.c_void_p()
        _lib.check(self.reg._lib.ndt_device_alloc(self.reg.ctx, max(1, points) * 16, C.byref(self.ptr)), self.reg.ctx)

    def upload(self, a):
        a = np.ascontiguousarray(a, np.float32)
        _lib.check(self.reg._lib.ndt_memcpy_h2d(self.reg.ctx, self.ptr, a.ctypes.data_as(C.c_void_p), a.nbytes), self.reg.ctx)

    def download(self, n):
        out = np.empty((n, 4), np.float32)
        _lib.check(self.reg._lib.ndt_synchronize(self.reg.ctx), self.reg.ctx)
        if n:
            _lib.check(self.reg._lib.ndt_memcpy_d2h(self.reg.ctx, out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes), self.reg.ctx)
        return out

    def free(self):
        self.reg._lib.ndt_device_free(self.reg.ctx, self.ptr)


@pytest.fixture(scope="module")
def scene():
    """12 keyframes of uniform random points in a 60 m cube (intensity 0..1), their Pose6D, and per keyframe the moved
    cloud as the restatement computes it (shared by every test, never modified)."""
    with xa.KeyframeMap() as probe:
        P = probe.geometry()["points_per_workgroup"]
    assert 256 <= P <= 4096
    sizes = [0, 0, 1, P - 1, 0, P, P + 1, 300, 2 * P + 1, 37, 0, 0]
    rng = np.random.default_rng(41)
    keyframes = [np.concatenate([rng.uniform(-30, 30, (n, 3)), rng.uniform(0, 1, (n, 1))], 1).astype(np.float32) for n in sizes]
    poses = [tuple(np.concatenate([rng.uniform(-5, 5, 3), rng.uniform(-0.2, 0.2, 2), rng.uniform(-np.pi, np.pi, 1)])) for _ in sizes]
    moved = []
    for k, p in zip(keyframes, poses):
        T = R.get_transformation(*p)
        assert np.array_equal(T, xa.icp.get_transformation(*p))
        moved.append(np.concatenate([R.transform_f32(T, k[:, :3]), k[:, 3:4]], 1).astype(np.float32))
    return {"P": P, "sizes": sizes, "keyframes": keyframes, "poses": poses, "moved": moved}


@pytest.fixture(scope="module")
def store(scene):
    with xa.KeyframeMap() as m:
        for i, k in enumerate(scene["keyframes"]):
            assert m.add(k) == i
        assert len(m) == 12 and m.num_points == sum(scene["sizes"])
        yield m


def stack_ref(scene, sel):
    return np.concatenate([scene["moved"][i] for i in sel] + [np.zeros((0, 4), np.float32)]).astype(np.float32)


# ---------------------------------------------------------------------------------------------- 1. stack parity
def selections(scene):
    sizes = scene["sizes"]
    return {"all": list(range(12)),
            "single": [8],
            "repeated": [3, 6, 3, 3],
            "descending": list(range(11, -1, -1)),
            # 300, 1, 37, 0 and P - 1 points: four boundaries strictly inside the first workgroup's P points
            "inside": [7, 2, 9, 4, 3, 8],
            "one_point": [2],
            "empty_only": [0, 1, 4]}


@pytest.mark.parametrize("name", ["all", "single", "repeated", "descending", "inside", "one_point", "empty_only"])
def test_stack_parity(scene, store, name):
    sel = selections(scene)[name]
    want = stack_ref(scene, sel)
    got = store.build([scene["poses"][i] for i in sel], sel, leaf=0.0)
    assert not store.overflowed
    assert same_bits(got, want), name
    g = store.geometry()
    P = scene["P"]
    assert g["points_per_workgroup"] == P and g["segments"] == len(sel)
    assert g["workgroups"] == (min(-(-len(want) // P), 2048) if len(want) else 0)
    assert store.count(sel) == len(want)
    if name == "all":
        assert g["workgroups"] > 1 and g["segments"] > g["workgroups"]
    if name == "inside":
        ends = np.cumsum([scene["sizes"][i] for i in sel])
        assert sum(0 < e < P for e in set(ends.tolist())) >= 3 and g["workgroups"] > 1
    # indices None = 0 .. n_sel - 1
    if name == "all":
        assert same_bits(store.build(scene["poses"], None, leaf=0.0), want)


def test_stack_equals_per_keyframe_transform_device(scene, store):
    """ndt_transform_device of each keyframe on its own, concatenated: the same bits as one k_map_stack launch."""
    lib, reg = store._lib, store.registration
    parts = []
    for k, p in zip(scene["keyframes"], scene["poses"]):
        buf = DeviceBuffer(store, len(k))
        try:
            buf.upload(k)
            T = np.ascontiguousarray(xa.icp.get_transformation(*p).T).reshape(-1)
            assert lib.ndt_transform_device(reg.ctx, _fp(T), buf.ptr, len(k), buf.ptr) == _lib.NDT_OK
            parts.append(buf.download(len(k)))
        finally:
            buf.free()
    per_keyframe = np.concatenate(parts)
    assert same_bits(per_keyframe, stack_ref(scene, range(12)))
    assert same_bits(store.build(scene["poses"], None, leaf=0.0), per_keyframe)


# ---------------------------------------------------------------------------------------------- 2. map parity
def test_map_parity(scene, store):
    oracle_lib.build_oracle()
    sel = list(range(12))
    stack = stack_ref(scene, sel)
    got = store.build(scene["poses"], None, leaf=0.5)
    assert not store.overflowed and 0 < len(got) < len(stack)
    assert same_bits(got, xa.voxel_downsample(stack, 0.5))
    assert same_bits(got, oracle_lib.voxel_downsample(stack, 0.5))
    # to_host=False: the map's own buffer
    ptr, n = store.build(scene["poses"], None, leaf=0.5, to_host=False)
    assert n == len(got) and ptr
    out = np.empty((n, 4), np.float32)
    _lib.check(store._lib.ndt_map_get(store._handle, _fp(out), n, None), store.ctx)
    assert same_bits(out, got)


def test_the_three_selections(scene, store):
    poses = scene["poses"]
    built = {}

    def from_indices(m, idx, all_poses):
        return m.build([all_poses[i] for i in idx], idx, leaf=0.5)

    assert same_bits(store.global_map(poses), from_indices(store, list(range(12)), poses))
    assert store.preview_indices() == [0, 2, 4, 6, 8, 10]
    assert same_bits(store.preview_map(poses), from_indices(store, [0, 2, 4, 6, 8, 10], poses))
    assert same_bits(store.preview_map(poses), xa.voxel_downsample(stack_ref(scene, [0, 2, 4, 6, 8, 10]), 0.5))
    assert store.submap_indices(0, 2) == [0, 1, 2] and store.submap_indices(11, 2) == [9, 10, 11]
    for root, idx in ((0, [0, 1, 2]), (11, [9, 10, 11]), (6, [4, 5, 6, 7, 8])):
        assert same_bits(store.submap(poses, root, search_num=2), from_indices(store, idx, poses)), root
    assert same_bits(store.submap(poses, 6, search_num=2), xa.voxel_downsample(stack_ref(scene, [4, 5, 6, 7, 8]), 0.5))
    # stores of one and of two (non-empty) keyframes: the preview stops one short of the last keyframe
    for n_kf, want_idx in ((1, []), (2, [0])):
        with xa.KeyframeMap(registration=store.registration) as small:
            picked = [5, 6][:n_kf]
            for i in picked:
                small.add(scene["keyframes"][i])
            sub_poses = [poses[i] for i in picked]
            assert small.preview_indices() == want_idx
            got = small.preview_map(sub_poses)
            want = xa.voxel_downsample(stack_ref(scene, [picked[i] for i in want_idx]), 0.5) if want_idx else np.zeros((0, 4), np.float32)
            assert same_bits(got, want), n_kf
            assert same_bits(small.global_map(sub_poses), xa.voxel_downsample(stack_ref(scene, picked), 0.5))
            built[n_kf] = len(got)
    assert built[1] == 0 and built[2] > 0
    with pytest.raises(ValueError):
        store.global_map(poses[:-1])


# ---------------------------------------------------------------------------------------------- 3. growth
def test_growth_keeps_every_keyframe(scene):
    with xa.KeyframeMap() as m:
        m.reserve(64)
        caps = [m.capacity]
        assert caps[0] == 64 and m.num_points == 0
        order = [2, 9, 7, 0, 3, 5, 1, 6, 8, 4, 10, 11]   # small keyframes first: several growth steps
        dev = DeviceBuffer(m, len(scene["keyframes"][6]))
        try:
            for slot, i in enumerate(order):
                k = scene["keyframes"][i]
                if i == 6:   # one keyframe arrives from a device buffer
                    dev.upload(k)
                    assert m.add_device(dev.ptr.value, len(k)) == slot
                else:
                    assert m.add(k) == slot
                if m.capacity != caps[-1]:
                    caps.append(m.capacity)
            assert len(caps) >= 3 and caps == sorted(caps), caps
            assert m.capacity >= m.num_points == sum(scene["sizes"]) and len(m) == 12
            for slot, i in enumerate(order):
                assert same_bits(m.keyframe(slot), scene["keyframes"][i]), (slot, i)
                assert m.keyframe_device(slot)[1] == scene["sizes"][i]
            got = m.build([scene["poses"][i] for i in order], None, leaf=0.0)
            assert same_bits(got, stack_ref(scene, order))
            # selection by slot: the build of test 1's "all", from the grown arena
            slot_of = {i: s for s, i in enumerate(order)}
            sel = [slot_of[i] for i in range(12)]
            assert same_bits(m.build(scene["poses"], sel, leaf=0.0), stack_ref(scene, range(12)))
            # a stored keyframe feeds Scan Context on the same context without a transfer
            slot = slot_of[8]
            ptr, n = m.keyframe_device(slot)
            with xa.SCManager(registration=m.registration) as sc:
                a = sc.makeAndSaveScancontextAndKeysDevice(ptr, n)
                b = sc.makeAndSaveScancontextAndKeys(scene["keyframes"][8][:, :3])
                da, db = sc.polarcontext(a), sc.polarcontext(b)
                assert da.any() and np.array_equal(da.view(np.uint64), db.view(np.uint64))
                assert np.array_equal(sc.ringkey(a).view(np.uint32), sc.ringkey(b).view(np.uint32))
        finally:
            dev.free()


# ---------------------------------------------------------------------------------------------- 4. overflow
def test_leaf_overflow_returns_the_stack(scene, store):
    """A 60 m scene at leaf 0.01 has 6000^3 cells, more than 2^31: pcl::VoxelGrid outputs its input."""
    stack = stack_ref(scene, range(12))
    assert np.prod(np.floor(np.ptp(stack[:, :3].astype(np.float64), axis=0) / 0.01) + 1.0) > 2.0 ** 31
    T = np.concatenate([np.ascontiguousarray(xa.icp.get_transformation(*p).T).reshape(-1) for p in scene["poses"]]).astype(np.float32)
    n_out = C.c_size_t()
    st = store._lib.ndt_map_build(store._handle, None, _fp(T), 12, 0.01, None, 0, C.byref(n_out))
    assert st == _lib.NDT_EOVERFLOW and n_out.value == len(stack)
    out = np.empty((len(stack), 4), np.float32)
    assert store._lib.ndt_map_get(store._handle, _fp(out), len(out), None) == _lib.NDT_OK
    assert same_bits(out, stack)
    got = store.build(scene["poses"], None, leaf=0.01)
    assert store.overflowed and same_bits(got, stack)
    store.build(scene["poses"], None, leaf=0.5)
    assert not store.overflowed


# ---------------------------------------------------------------------------------------------- 5. destinations
def test_destinations(scene):
    poses = scene["poses"]
    with xa.KeyframeMap() as m:
        for k in scene["keyframes"]:
            m.add(k)
        p, n = C.c_void_p(), C.c_size_t()
        assert m._lib.ndt_map_result(m._handle, C.byref(p), C.byref(n)) == _lib.NDT_EINVAL   # no internal build yet
        assert "own buffer" in last_error(m)
        sel_a, sel_b = [3, 5, 6], [8, 7, 9, 2]
        inner = m.build([poses[i] for i in sel_a], sel_a, leaf=0.5)
        p0, n0 = m.build([poses[i] for i in sel_a], sel_a, leaf=0.5, to_host=False)
        a, b = DeviceBuffer(m, m.count(sel_a)), DeviceBuffer(m, m.count(sel_b))
        try:
            na = m.build_into(a.ptr.value, a.points, [poses[i] for i in sel_a], sel_a, leaf=0.5)
            nb = m.build_into(b.ptr.value, b.points, [poses[i] for i in sel_b], sel_b, leaf=0.5)
            got_a, got_b = a.download(na), b.download(nb)   # read after both builds: neither disturbed the other
            assert same_bits(got_a, inner)
            assert same_bits(got_a, xa.voxel_downsample(stack_ref(scene, sel_a), 0.5))
            assert same_bits(got_b, xa.voxel_downsample(stack_ref(scene, sel_b), 0.5))
            # the stacked cloud itself lands in a caller buffer directly
            ns = m.build_into(b.ptr.value, b.points, [poses[i] for i in sel_b], sel_b, leaf=0.0)
            assert ns == b.points and same_bits(b.download(ns), stack_ref(scene, sel_b))
            # builds into caller buffers leave the map's own result as it was
            assert m._lib.ndt_map_result(m._handle, C.byref(p), C.byref(n)) == _lib.NDT_OK
            assert (p.value, n.value) == (p0, n0)
            out = np.empty((n0, 4), np.float32)
            assert m._lib.ndt_map_get(m._handle, _fp(out), n0, None) == _lib.NDT_OK
            assert same_bits(out, inner)
        finally:
            a.free()
            b.free()


# ---------------------------------------------------------------------------------------------- 6. loop closure from a store
def same_refine(a, b):
    assert set(a) == set(b)
    for key in a:
        if key == "history":
            assert len(a[key]) == len(b[key])
            for ha, hb in zip(a[key], b[key]):
                assert ha["pairs"] == hb["pairs"] and ha["state"] == hb["state"] and ha["mse"] == hb["mse"]
                assert same_bits(ha["T"], hb["T"])
        elif isinstance(a[key], np.ndarray):
            assert same_bits(a[key], b[key]), key
        else:
            assert a[key] == b[key], key


@pytest.mark.parametrize("literal_root", [False, True])
def test_refine_loop_from_a_store(literal_root):
    from test_gpu_icp import loop_keyframes
    keyframes, poses, _ = loop_keyframes()
    args = dict(loop_idx=0, curr_idx=11, search_num=2, leaf=0.5, literal_root=literal_root, return_clouds=True)
    want = xa.refine_loop(keyframes, poses, **args)
    assert want["accepted"] and want["n_target"] > want["n_source"] > 0
    with xa.KeyframeMap() as m:
        for k in keyframes:
            m.add(k)
        same_refine(xa.refine_loop(keyframes, poses, store=m, **args), want)
        same_refine(xa.refine_loop(None, poses, store=m, **args), want)   # the store alone is enough
        with pytest.raises(ValueError):
            xa.refine_loop(None, poses, store=m, loop_idx=0, curr_idx=12)


def test_close_loops_from_a_store():
    """The first 80 keyframes of test_gpu_scancontext.test_close_loops' route: its two earliest candidates, (0, 78) and
    (0, 79), both inside the 20 m gate."""
    import sc_restate
    import sc_scene
    scans, truth = sc_scene.route_keyframes(4200)
    scans, truth = scans[:80], truth[:80]
    scans = [np.delete(s, sc_restate.bin_sensitive(s), axis=0) for s in scans]
    rng = np.random.default_rng(17)
    keyframes = [np.concatenate([s, rng.uniform(0, 1, (len(s), 1)).astype(np.float32)], 1) for s in scans]
    amp = np.array([0.3, 0.3, 0.05, np.radians(0.5), np.radians(0.5), np.radians(1.0)])
    poses = [tuple(np.array(p) + rng.uniform(-1, 1, 6) * amp) for p in truth]
    detect = dict(dist_thres=0.4, tree_making_period=1)
    refine = dict(search_num=25, leaf=0.5)
    want = xa.close_loops(keyframes, poses, detect_args=detect, **refine)
    assert sorted([(a[0], a[1]) for a in want[0]] + [(r[0], r[1]) for r in want[1]]) == [(0, 78), (0, 79)]

    def same(got):
        assert got[1] == want[1] and len(got[0]) == len(want[0])
        for g, w in zip(got[0], want[0]):
            assert g[:2] == w[:2] and same_bits(g[2], w[2]) and g[3] == w[3]

    same(xa.close_loops(keyframes, poses, detect_args=detect, store=True, **refine))
    with xa.KeyframeMap() as m:
        for k in keyframes:
            m.add(k)
        same(xa.close_loops(None, poses, detect_args=detect, store=m, **refine))


def test_add_strided_records(scene):
    """ndt_map_add over 32-byte records with the intensity at float 4 (pcl::PointXYZI's layout, the padding poisoned)
    stores the keyframe the packed (N, 4) call stores."""
    cloud = scene["keyframes"][7]
    assert len(cloud) == 300
    wide = np.full((len(cloud), 8), np.nan, np.float32)
    wide[:, :3] = cloud[:, :3]
    wide[:, 4] = cloud[:, 3]
    with xa.KeyframeMap() as m:
        assert m.add(cloud) == 0
        idx = C.c_int(-1)
        assert m._lib.ndt_map_add(m._handle, _fp(wide), len(wide), 32, 4, C.byref(idx)) == _lib.NDT_OK and idx.value == 1
        assert m.num_points == 600
        assert same_bits(m.keyframe(0), cloud) and same_bits(m.keyframe(1), m.keyframe(0))


# ---------------------------------------------------------------------------------------------- 7. argument errors
def test_argument_errors(scene, store):
    """Plain argument checks: each is refused before anything is launched."""
    lib, h = store._lib, store._handle
    T = np.tile(np.eye(4, dtype=np.float32).reshape(-1), 12)
    n_out = C.c_size_t()
    total = store.count(None)
    buf = DeviceBuffer(store, total)
    try:
        for bad in (-1, len(store)):
            idx = np.array([3, bad], np.int32)
            assert lib.ndt_map_build(h, _ip(idx), _fp(T), 2, 0.5, None, 0, C.byref(n_out)) == _lib.NDT_EINVAL
            assert "out of range" in last_error(store)
            cnt = C.c_longlong()
            assert lib.ndt_map_count(h, _ip(idx), 2, C.byref(cnt)) == _lib.NDT_EINVAL
            assert lib.ndt_map_keyframe(h, bad, None, None) == _lib.NDT_EINVAL
            assert "out of range" in last_error(store)
        assert lib.ndt_map_build(h, None, _fp(T), 13, 0.5, None, 0, C.byref(n_out)) == _lib.NDT_EINVAL   # NULL = 0..12: one too many
        assert lib.ndt_map_build(h, None, _fp(T), 12, 0.5, buf.ptr, total - 1, C.byref(n_out)) == _lib.NDT_EINVAL
        assert "too small" in last_error(store)
        assert lib.ndt_map_build(h, None, None, 12, 0.5, None, 0, C.byref(n_out)) == _lib.NDT_EINVAL
        assert "null poses" in last_error(store)
        assert lib.ndt_map_build(h, None, _fp(T), 12, -1.0, None, 0, C.byref(n_out)) == _lib.NDT_EINVAL
        assert lib.ndt_map_build(h, None, _fp(T), -1, 0.5, None, 0, C.byref(n_out)) == _lib.NDT_EINVAL
        assert lib.ndt_map_build(h, None, _fp(T), 12, 0.5, None, 0, None) == _lib.NDT_EINVAL
        assert lib.ndt_map_reserve(h, -1) == _lib.NDT_EINVAL
        assert lib.ndt_map_add(h, _fp(T), 4, 12, 3, None) == _lib.NDT_EINVAL      # stride below one float4
        assert lib.ndt_map_add_device(h, None, 4, None) == _lib.NDT_EINVAL
        assert len(store) == 12   # nothing was added by the refused calls
        # an empty selection and a selection of empty keyframes: NDT_OK, nothing written
        n_out.value = 99
        assert lib.ndt_map_build(h, None, None, 0, 0.5, None, 0, C.byref(n_out)) == _lib.NDT_OK and n_out.value == 0
        idx = np.array([0, 1, 4], np.int32)
        n_out.value = 99
        assert lib.ndt_map_build(h, _ip(idx), _fp(T), 3, 0.5, buf.ptr, 0, C.byref(n_out)) == _lib.NDT_OK and n_out.value == 0
        assert store.build([], [], leaf=0.5).shape == (0, 4)
        # NULL handles
        assert lib.ndt_map_size(None) == -1 and lib.ndt_map_build(None, None, None, 0, 0.5, None, 0, C.byref(n_out)) == _lib.NDT_EINVAL
        with pytest.raises(ValueError):
            store.add(np.zeros((3, 3), np.float32))
        with pytest.raises(ValueError):
            store.build(scene["poses"][:3], [1, 2], leaf=0.5)
    finally:
        buf.free()
