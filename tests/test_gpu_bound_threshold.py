"""The FP32 prefilter's threshold from the bound (srl_kernels.hip: thr_from_bound; srl_debug_set_bound_culling modes 0 / 1 / 2).

A pass that starts from bounds takes the squared cull radius r^2 as the upper bound of the K-th smallest FP32 distance and searches for
no threshold: mode 1.  Mode 2 uses the bounds for the voxel cull only and searches (what the library did before), mode 0 uses no
bounds.  The selection stays the exact FP64 top-K of the reference (optimize.cpp:365-426), so NOTHING observable may differ between the
modes, and every pass equals the oracle:
  1. dense scene, 2 999 keypoints (an odd tail pair), five poses with a jump, taps on / off, plain and armed launches: bit for bit;
  2. more survivors under r^2 than the pair finish (32) or the single finish (64) takes: the search runs after all;
  3. pairs of a keypoint with a bound and one without (fewer than K candidates; a voxel face crossed);
  4. ties inside the radius: the heap replay decides;
  5. the dense scene with voxel keys near +-32 000 (an FP32 ulp of 2 mm);
  6. init mode (r = 2, the looped path): three passes, and the two-loop fallback at more than 64 survivors;
  7. the banded threshold search of the single-keypoint paths (cand_select, the loop's tail): both ends of the band, the fallback."""
import numpy as np
import pytest

import sr_livo_amd as srl
from sr_livo_amd import capi, synth
from test_gpu_bound_culling import _poses, _same
from test_gpu_bound_culling_sparse import _crossing_cell, _plain_rule_drops
from test_gpu_eigen_stress import _voxelise

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
K = 20
Q0 = np.array([1.0, 0.0, 0.0, 0.0])
T_LAST = np.array([0.0, 0.0, 30.0])


# ------------------------------------------------------------------------------------------------ passes: device and oracle
def _device_passes(ctx, raw, poses, mode, armed=0, frame_id=100, t_last=T_LAST, taps=True, opts=None):
    opts = opts or srl.default_opts(max_num_residuals=INT_MAX)
    ctx.set_armed_launch(armed)
    ctx.set_bound_culling(mode)
    ctx.sweep_upload(raw)                 # a new sweep: no bounds from earlier runs
    ctx.set_taps(1 if taps else 0)
    out = []
    for q, t in poses:
        neq, rc = ctx.build_residuals(capi.make_frame(q, t, t_last, frame_id=frame_id), opts)
        ids, status, ncand = (a.copy() for a in ctx.fetch_neighbors(K=K)) if taps else (None, None, None)
        out.append(dict(neq=neq, ids=ids, status=status, ncand=ncand))
    ctx.set_taps(0)
    ctx.set_armed_launch(1)
    ctx.set_bound_culling(1)
    return out


def _oracle_passes(oracle_lib, m, raw, poses, frame_id=100, t_last=T_LAST):
    oo = oracle_lib.default_opts(max_num_residuals=INT_MAX)
    return [m.build_plane_residuals(oo, raw, q, t, t_last, frame_id=frame_id) for q, t in poses]


def _check_modes_against_oracle(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, frame_id=100, modes=(0, 1, 2)):
    """every pass of every mode: the oracle's ids, status and candidate total; mode 1 hands no more keypoints to the general path than mode 2"""
    m = oracle_lib.Map(oracle_backend)
    m.import_(keys, counts, xyz)
    orc = _oracle_passes(oracle_lib, m, raw, poses, frame_id)
    ctx.map_upload(keys, counts, xyz)
    got = {mode: _device_passes(ctx, raw, poses, mode, frame_id=frame_id) for mode in modes}
    for mode in modes:
        for k, (g, o) in enumerate(zip(got[mode], orc)):
            bad = np.flatnonzero((g["ids"] != o["ids"]).any(1))
            assert bad.size == 0, ("ids differ from the oracle", mode, k, bad[:8])
            assert np.array_equal(g["status"], o["status"]), (mode, k)
            assert g["neq"].sum_candidates == o["neq"].sum_candidates and g["neq"].num_residuals == o["neq"].num_residuals, (mode, k)
    if 1 in modes and 2 in modes:
        # The threshold from the bound never sends a keypoint to the general path that the search would have finished (more survivors than
        # the finish takes: searched in place).  The other way round it can happen on sparse maps: the search works on per-lane minima
        # and may end on a looser threshold than r^2, with more than 64 survivors where r^2 leaves at most 64.  (Dense scenes: equal,
        # test_modes_agree_bit_for_bit.)
        assert all(a["neq"].num_fallback <= b["neq"].num_fallback for a, b in zip(got[1], got[2]))
    return orc, got


def _r2_of_bound(flat, ids_prev, p_prev, p_now):
    """the squared radius a pass takes from the bound, without its slack (a lower bound of phase 0's r^2)"""
    tau = ((flat[ids_prev[:, K - 1]] - p_prev) ** 2).sum(1)
    return (np.sqrt(tau) + np.linalg.norm(p_now - p_prev, axis=1)) ** 2


@pytest.fixture(scope="module")
def ctx():
    c = srl.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ 1. the modes agree bit for bit
@pytest.fixture(scope="module")
def dense():
    cands, L = synth.map_candidates(5501, 200_000)
    c = srl.Context(0)
    c.map_insert(cands)
    sw = synth.make_sweep(5502, 2_999, L)
    yield dict(ctx=c, cands=cands, L=L, sw=sw)
    c.close()


@pytest.mark.parametrize("taps", [True, False])
def test_modes_agree_bit_for_bit(dense, taps):
    c, sw = dense["ctx"], dense["sw"]
    poses = _poses(sw, 5, 1, jump=3)
    ref = _device_passes(c, sw["raw"], poses, 0, 0, t_last=sw["t_last"], taps=taps)
    for armed in (0, 2):
        got = {mode: _device_passes(c, sw["raw"], poses, mode, armed, t_last=sw["t_last"], taps=taps) for mode in (1, 2)}
        for mode in (1, 2):
            for k, (g, r) in enumerate(zip(got[mode], ref)):
                _same((g["neq"], g["ids"]), (r["neq"], r["ids"]), (mode, armed, k))
        assert [g["neq"].num_fallback for g in got[1]] == [g["neq"].num_fallback for g in got[2]], armed


# ------------------------------------------------------------------------------------------------ 2. overflow of the two finishes
_OCTANTS = [(1, 1, 1), (-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1)]


def _corner_cluster(rng, corner, nvox, radius=0.02):
    """nvox of the eight voxels that meet in `corner`, 20 points each within `radius` (per axis) of it"""
    return np.concatenate([corner + np.array(s) * rng.uniform(0.002, radius, (20, 3)) for s in _OCTANTS[:nvox]])


def _dense_block(rng, lo):
    """2 x 2 x 2 full voxels (eight occupied voxels: the pair path), and a keypoint near their common corner"""
    pts = np.concatenate([lo + np.array([i, j, k]) + rng.uniform(0.02, 0.98, (20, 3)) for i in range(2) for j in range(2) for k in range(2)])
    return pts, lo + 1.0 + rng.uniform(0.05, 0.25, 3)


def _overflow_scene(seed):
    """keypoints 0 / 2 / 4 sit in the corner where 3 / 5 / 5 clustered voxels meet (60 / 100 / 100 points within centimetres), 1 and 3
    are ordinary dense keypoints: two pairs and the odd keypoint (the single-keypoint path).  The second pose moves everything 0.3 m."""
    rng = np.random.default_rng(seed)
    pts, kps = [], []
    for i, nvox in enumerate((3, 5, 5)):
        corner = np.array([10.0 + 8 * i, 10.0, 10.0])
        pts.append(_corner_cluster(rng, corner, nvox))
        kps.append(corner + 0.001)
        if i < 2:
            P, kp = _dense_block(rng, np.array([10.0 + 8 * i, 30.0, 10.0]))
            pts.append(P); kps.append(kp)
    step = 0.3 * np.array([1.0, 1.0, 1.0]) / np.sqrt(3.0)
    return np.concatenate(pts).astype(np.float32), np.array(kps), [(Q0, np.zeros(3)), (Q0, step), (Q0, step)]


@pytest.mark.parametrize("frame_id", [100, 5])
def test_more_survivors_under_the_bound_than_a_finish_takes(ctx, oracle_lib, oracle_backend, frame_id):
    pts, raw, poses = _overflow_scene(61)
    keys, counts, xyz = _voxelise(pts)
    orc, got = _check_modes_against_oracle(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, frame_id=frame_id)
    # the scene does what it is meant to: small tau, large r -- candidates within the bound's radius of the moved keypoint
    flat = xyz.reshape(-1, 3).astype(np.float64)
    p0, p1 = raw + poses[0][1], raw + poses[1][1]
    r2 = _r2_of_bound(flat, orc[0]["ids"], p0, p1)
    live = flat[(np.arange(len(flat)) % K) < np.repeat(counts, K)]
    within = np.array([int((((live - p) ** 2).sum(1) <= r).sum()) for p, r in zip(p1, r2)])
    print("candidates within the bound:", within, "sqrt(tau):", np.sqrt(((flat[orc[0]["ids"][:, K - 1]] - p0) ** 2).sum(1)))
    assert 32 < within[0] <= 64 and within[2] > 64 and within[4] > 64, within


# ------------------------------------------------------------------------------------------------ 3. mixed pairs
def test_pairs_of_a_keypoint_with_a_bound_and_one_without(ctx, oracle_lib, oracle_backend):
    """pair (0, 1): dense + a keypoint with 12 candidates in all (no K-th neighbour, tau = +inf); pair (2, 3) and (4, 5): dense + a keypoint
    that crosses a voxel face with its K nearest one voxel edge away (test_gpu_bound_culling_sparse's construction: the bound is dropped,
    and would lose neighbours if it were not); both orders inside the pair"""
    rng = np.random.default_rng(62)
    pts, kps = [], []
    P, kp = _dense_block(rng, np.array([40.0, 40.0, 40.0])); pts.append(P); kps.append(kp)
    lone = np.array([60.5, 40.5, 40.5])
    pts.append(lone + rng.uniform(-0.3, 0.3, (12, 3))); kps.append(lone + 0.05)
    for i in range(2):
        P, kp = _dense_block(rng, np.array([40.0, 50.0 + 10 * i, 40.0]))
        ck, CP = _crossing_cell(rng, 12, 1, 10 + 8 * i, 10 + 3 * i, partial=bool(i))
        pts += [P, CP]
        kps += [kp, ck] if i == 0 else [ck, kp]
    raw = np.array(kps)
    keys, counts, xyz = _voxelise(np.concatenate(pts).astype(np.float32))
    step = np.array([-0.06, 0.0, 0.0])
    poses = [(Q0, np.zeros(3)), (Q0, step), (Q0, step), (Q0, np.zeros(3)), (Q0, step)]
    orc, got = _check_modes_against_oracle(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses)
    assert (orc[0]["ids"][1] >= 0).sum() == 12
    for k in (1, 4):        # the crossings: the plain rule (no condition on the region) would drop neighbours of keypoints 3 and 4
        drops = _plain_rule_drops(keys, xyz, 1.0, raw, poses[k - 1], orc[k - 1]["ids"], poses[k], orc[k]["ids"])
        assert drops[3] > 0 and drops[4] > 0 and drops[0] == 0 and drops[2] == 0 and drops[5] == 0, (k, drops)


# ------------------------------------------------------------------------------------------------ 4. ties inside the radius
def test_ties_inside_the_radius_are_replayed(ctx, oracle_lib, oracle_backend):
    """keypoint 0: ranks K - 1 and K at EXACTLY the same distance (0.25 m either side); keypoint 2: the two 2^-54 m apart in distance
    (squared distances closer than 1 + 2^-50: one sqrt for the reference); keypoints 1 and 3: ordinary partners.  Three passes with
    small steps across the tie direction: the replay decides every time, the tied keypoints never get a bound."""
    rng = np.random.default_rng(63)
    pts, kps = [], []
    for i, eps in enumerate((0.0, 2.0 ** -54)):
        c = np.array([0.375, 20.5 + 8 * i, 20.875])
        # 19 nearer points, two of them in the voxel above: the home voxel holds 17 + 2 tied = 19 of the 20 a voxel takes
        near = np.concatenate([c + rng.uniform(-0.12, 0.12, (17, 3)), c + np.array([[0.01, 0.02, 0.15], [-0.03, 0.01, 0.17]])])
        tied = np.array([c + [0.5, 0, 0], c - [0.5, 0, 0]])                # x = 0.875 and -0.125: exact in FP32
        far = c + np.array([[0, 0.7, 0], [0, -0.7, 0.1], [0.1, 0, 0.7]])
        pts.append(np.concatenate([near, tied, far]))
        kps.append(c + [eps, 0, 0])
        P, kp = _dense_block(rng, np.array([30.0, 20.0 + 8 * i, 20.0])); pts.append(P); kps.append(kp)
    raw = np.array(kps)
    pts32 = np.concatenate(pts).astype(np.float32)
    d = pts32[19:21].astype(np.float64) - raw[0]
    assert (d[0] ** 2).sum() == (d[1] ** 2).sum()
    off = sum(len(p) for p in pts[:2])
    d = pts32[off + 19: off + 21].astype(np.float64) - raw[2]
    a, b = sorted(((d[0] * d[0])[0] + (d[0] * d[0])[1] + (d[0] * d[0])[2], (d[1] * d[1])[0] + (d[1] * d[1])[1] + (d[1] * d[1])[2]))
    assert a < b <= a * (1 + 2.0 ** -51), (a, b)
    keys, counts, xyz = _voxelise(pts32)
    poses = [(Q0, np.zeros(3))] * 3                                        # (a moved pose would break the ties)
    orc, got = _check_modes_against_oracle(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses)
    for mode in (1, 2):
        assert all(g["neq"].num_fallback >= 2 for g in got[mode]), [g["neq"].num_fallback for g in got[mode]]
    # and with a step that keeps keypoint 0's tie (along y: both tied points stay equally far)
    poses = [(Q0, np.zeros(3)), (Q0, np.array([0.0, 0.03, 0.0])), (Q0, np.array([0.0, 0.05, 0.0]))]
    _check_modes_against_oracle(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses)


# ------------------------------------------------------------------------------------------------ 5. magnitude
def test_keys_near_the_end_of_the_int16_range(dense, oracle_lib, oracle_backend):
    L, sw = dense["L"], dense["sw"]
    far = float(np.floor(32_700.0 - L - 60.0))                             # the sweep reaches 50 m beyond the sensor
    assert far > 32_000 - 200
    shift = np.array([far, -far, 100.0])
    m = oracle_lib.Map(oracle_backend)
    m.add_points(dense["cands"] + shift)
    keys, counts, xyz = m.export()
    assert np.abs(keys.astype(np.int64)).max() > 32_000 - 200
    poses = [(q, t + shift) for q, t in _poses(sw, 3, 1)]
    t_last = sw["t_last"] + shift
    orc = _oracle_passes(oracle_lib, m, sw["raw"], poses, t_last=t_last)
    c = srl.Context(0)
    try:
        c.map_upload(keys, counts, xyz)
        for mode in (1, 2):
            got = _device_passes(c, sw["raw"], poses, mode, t_last=t_last)
            for k, (g, o) in enumerate(zip(got, orc)):
                assert np.array_equal(g["ids"], o["ids"]) and np.array_equal(g["status"], o["status"]), (mode, k)
                assert g["neq"].sum_candidates == o["neq"].sum_candidates, (mode, k)
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------ 6. init mode
def test_init_mode_modes_agree_bit_for_bit(dense):
    c, sw = dense["ctx"], dense["sw"]
    poses = _poses(sw, 3, 5)
    ref = _device_passes(c, sw["raw"], poses, 0, frame_id=5, t_last=sw["t_last"])
    got = {mode: _device_passes(c, sw["raw"], poses, mode, frame_id=5, t_last=sw["t_last"]) for mode in (1, 2)}
    for mode in (1, 2):
        for k, (g, r) in enumerate(zip(got[mode], ref)):
            _same((g["neq"], g["ids"]), (r["neq"], r["ids"]), (mode, k))
    assert [g["neq"].num_fallback for g in got[1]] == [g["neq"].num_fallback for g in got[2]]
# (the crafted keypoint with more than 64 survivors under r^2 in init mode: test_more_survivors_under_the_bound_than_a_finish_takes[5])


# ------------------------------------------------------------------------------------------------ 7. the banded single-keypoint search
def _sparse_scene(seed):
    """test_gpu_band_bisection's sparse map with six layers: all 27 voxels around a keypoint hold one to three points (nine candidate
    rounds: cand_select), the K-th neighbour 1.2 ... 2.5 m away -- squared distances on either side of 2 m^2, the band's upper end"""
    rng = np.random.default_rng(seed)
    pts = []
    for ix in range(-8, 8):
        for iy in range(-8, 8):
            for iz in range(-3, 3):
                for _ in range(int(rng.integers(1, 4))):
                    pts.append(np.array([ix, iy, iz]) + rng.uniform(0.02, 0.98, 3))
    raw = rng.uniform([-6, -6, -1.8], [6, 6, 1.8], size=(1500, 3))
    return np.array(pts, np.float32), raw


def _tiny_scene(seed):
    """20 points inside a 4 mm ball around every keypoint -- every squared distance below 2^-15 m^2, the band's lower end -- and 13 far,
    full voxels around its home voxel: 14 occupied voxels, five candidate rounds, so that the keypoint is selected by cand_select"""
    rng = np.random.default_rng(seed)
    offs = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)][:13]
    pts, kps = [], []
    for n in range(257):                                                   # (odd: the last keypoint has no partner)
        c = np.array([(n % 16) * 4 + 2.5, (n // 16) * 4 + 2.5, 2.5])
        pts.append(c + rng.normal(0, 0.0012, (20, 3)))
        for o in offs:
            pts.append(c + np.array(o) * 1.0 + 0.3 * np.array(o) + rng.uniform(-0.15, 0.15, (20, 3)))      # the far part of the neighbour voxel
        kps.append(c + rng.normal(0, 0.0005, 3))
    return np.concatenate(pts).astype(np.float32), np.array(kps)


@pytest.mark.parametrize("frame_id", [100, 5])
@pytest.mark.parametrize("scene", ["sparse", "tiny"])
def test_banded_search_of_the_single_keypoint_paths(ctx, oracle_lib, oracle_backend, scene, frame_id):
    pts, raw = _sparse_scene(71) if scene == "sparse" else _tiny_scene(72)
    keys, counts, xyz = _voxelise(pts)
    poses = [(Q0, np.zeros(3)), (Q0, np.array([0.02, -0.01, 0.015]))]
    orc, got = _check_modes_against_oracle(ctx, oracle_lib, oracle_backend, keys, counts, xyz, raw, poses, frame_id=frame_id, modes=(1, 2))
    flat = xyz.reshape(-1, 3).astype(np.float64)
    ids = orc[0]["ids"]
    full = ids.min(1) >= 0
    d2_k = ((flat[ids[full][:, K - 1]] - raw[full]) ** 2).sum(1)
    if scene == "sparse":
        assert (d2_k > 2.0).sum() > 50 and (d2_k < 2.0).sum() > 50, (int((d2_k > 2.0).sum()), int((d2_k < 2.0).sum()))
        assert np.all(got[1][0]["ncand"] >= 27)                            # all 27 voxels occupied (one to three points each)
    else:
        assert np.mean(d2_k < 2.0 ** -15) > 0.9
        assert np.all(got[1][0]["ncand"] == 20 * 14)
