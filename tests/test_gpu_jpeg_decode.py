"""Baseline JPEG frames on the device (srl_jpeg_decode, srl_jpeg_download, srl_image_prepare_jpeg, srl_jpeg_idct_blocks; include/srlivo_hip.h
and srlivo_hip_debug.h) against tests/jpeg_checker.py, the independent restatement that tests/test_jpeg_checker_reference.py holds
bytewise to libjpeg-turbo's decode, and against the committed fixtures (Pillow's streams and Pillow's pixels).  Every comparison is
BYTEWISE: the decode is integer arithmetic on both sides.

Sizes are the smallest at which each rule can go wrong: 1 x 1; 8 x 9 (one chroma column: both edge rules of the upsampling meet in it);
33 x 17 and 37 x 43 (odd chroma sizes, partial MCUs at both edges); 16 x 16 and 40 x 48 (whole MCUs; 40 x 48 at 4:4:4 is 90 blocks: more
than one workgroup of the IDCT kernel, and 480 pixel groups: more than one of the colour kernel)."""
import ctypes as C
import functools

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_checker as ck
import sr_livo_amd as srl
from sr_livo_amd import capi

pytestmark = pytest.mark.gpu
SRL_OK, SRL_ERR_BAD_ARG, SRL_ERR_UNSUPPORTED, SRL_ERR_NO_MAP, SRL_ERR_NO_SWEEP = 0, -3, -4, -5, -6
GOLDEN = jc.load_golden()
L1_LIMIT = 14000                                           # SRL_JPEG_L1_INT32 of srl_jpeg.hip: the 32-bit IDCT runs up to it


@functools.lru_cache(maxsize=None)
def _want(name):
    out = ck.decode(GOLDEN[name][0])
    out.setflags(write=False)
    return out


def _same(name, got, want):
    want = np.ascontiguousarray(want)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (name, bad.size, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


@pytest.fixture(scope="module")
def ctx():
    c = srl.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ 1. whole frames
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_the_decoded_frame_equals_the_checker_and_the_fixture(ctx, name):
    data, pillow = GOLDEN[name]
    info = ctx.jpeg_decode(data)
    assert (info.rows, info.cols) == pillow.shape[:2]
    got = ctx.jpeg_download(info.rows, info.cols)
    _same(name + " vs the checker", got, _want(name))
    _same(name + " vs the fixture", got, pillow)
    # a strided download leaves the padding alone
    out = np.full((info.rows, 3 * info.cols + 7), 0xA5, np.uint8)
    ctx._chk(ctx.lib.srl_jpeg_download(ctx.h, capi._ptr(out), out.strides[0]), "srl_jpeg_download")
    assert np.array_equal(out[:, :3 * info.cols].reshape(info.rows, info.cols, 3), pillow) and np.all(out[:, 3 * info.cols:] == 0xA5)


def test_decoding_twice_gives_the_same_bytes_and_sizes_may_alternate(ctx):
    names = ["40x48_420_rrow", "1x1_gray_q35" if "1x1_gray_q35" in GOLDEN else [n for n in GOLDEN if n.startswith("1x1_gray")][0], "37x43_422_r2", "40x48_420_rrow"]
    first = {}
    for name in names + names:
        info = ctx.jpeg_decode(GOLDEN[name][0])
        got = ctx.jpeg_download(info.rows, info.cols).tobytes()
        assert first.setdefault(name, got) == got and got == GOLDEN[name][1].tobytes(), name


# ------------------------------------------------------------------------------------------------ 2. the IDCT alone
def _idct(ctx, coef, qt):
    coef = np.ascontiguousarray(coef, np.int16).reshape(-1, 64)
    got = ctx.jpeg_idct_blocks(coef, qt)
    _same("idct", got, ck.idct_blocks(coef, qt))
    return got


def test_idct_dc_only_blocks(ctx):
    coef = np.zeros((41, 64), np.int16)
    coef[:, 0] = np.linspace(-1200, 1200, 41).astype(np.int16)
    got = _idct(ctx, coef, np.full(64, 1, np.uint16))
    assert all(len(np.unique(b)) == 1 for b in got) and got[0, 0] == 0 and got[-1, 0] == 255 and got[20, 0] == 128


@pytest.mark.parametrize("q", [1, 255])
def test_idct_every_single_coefficient_small_and_at_the_ends_of_int16(ctx, q):
    """+-1 (the rounding of both passes) and +-32767: with table entry 255 the products reach 8.4e6, pass 2 leaves int32_t (the 64-bit
    form) and the results pass through the wrap branches of the range limit"""
    coef = np.zeros((4 * 64, 64), np.int16)
    for k in range(64):
        coef[4 * k:4 * k + 4, k] = (1, -1, 32767, -32767)
    qt = np.full(64, q, np.uint16)
    got = _idct(ctx, coef, qt)
    if q == 255:
        assert ck.block_l1(coef, qt) > L1_LIMIT
        # by the checker's own passes: results far beyond the table's period, and every branch of the range limit is taken
        d = coef.astype(np.int64).reshape(-1, 8, 8) * 255
        ws = np.stack(ck._pass([d[:, k, :] for k in range(8)], 11), axis=1)
        idx = np.stack(ck._pass([ws[:, :, k] for k in range(8)], 18), axis=2)
        assert np.max(np.abs(idx)) > 100 * 1024 and np.max(np.abs(ws)) * 27431 > 2 ** 31
        idx = idx & 0x3FF
        assert (idx < 128).any() and ((idx >= 128) & (idx < 512)).any() and ((idx >= 512) & (idx < 896)).any() and (idx >= 896).any()


def test_idct_at_the_edge_of_the_32_bit_guard_on_either_side(ctx):
    """blocks whose sum of |coef x table| is exactly the limit (the 32-bit form runs) and one above it (the 64-bit form): one large
    coefficient, the sum spread over the first row, over the first column, over everything, with signs that add up in the corner"""
    qt = np.full(64, 1, np.uint16)
    for total in (L1_LIMIT, L1_LIMIT + 1):
        blocks = []
        for k in (0, 1, 8, 9, 63):
            b = np.zeros(64, np.int64); b[k] = total; blocks.append(b); blocks.append(-b)
        row = np.zeros(64, np.int64); row[:8] = total // 8; row[0] += total - row.sum(); blocks.append(row)
        col = np.zeros(64, np.int64); col[::8] = total // 8; col[0] += total - col.sum(); blocks.append(col)
        every = np.full(64, total // 64, np.int64); every[0] += total - every.sum(); blocks.append(every); blocks.append(-every)
        alt = every * np.where((np.arange(64) // 8 + np.arange(64) % 8) % 2 == 0, 1, -1); blocks.append(alt)
        coef = np.array(blocks)
        assert ck.block_l1(coef, qt) == total and np.max(np.abs(coef)) <= 32767
        _idct(ctx, coef, qt)
    # the same sums reached through the table
    qt = np.full(64, 200, np.uint16)
    coef = np.zeros((2, 64), np.int16); coef[0, :7] = 10; coef[1, :7] = 10; coef[1, 7] = 1      # 14000 and 14200
    assert ck.block_l1(coef[:1], qt) == L1_LIMIT and ck.block_l1(coef, qt) > L1_LIMIT
    _idct(ctx, coef[:1], qt)
    _idct(ctx, coef, qt)


def test_idct_random_blocks(ctx):
    rng = np.random.default_rng(11)
    qt = rng.integers(1, 256, 64).astype(np.uint16)
    fine = rng.integers(1, 8, 64).astype(np.uint16)
    sparse = np.where(rng.random((300, 64)) < 0.2, rng.integers(-60, 61, (300, 64)), 0)
    sparse[:, 0] = rng.integers(-1024, 1024, 300) // fine[0]
    assert ck.block_l1(sparse, fine) <= L1_LIMIT
    _idct(ctx, sparse, fine)                                                     # what an encoder writes: the 32-bit form
    _idct(ctx, rng.integers(-2048, 2048, (333, 64)), qt)                         # dense and large: the 64-bit form
    _idct(ctx, rng.integers(-32768, 32768, (65, 64)), np.full(64, 255, np.uint16))
    # one block more than a workgroup's 32, and the two forms give the same bytes where both are valid
    small = rng.integers(-20, 21, (33, 64))
    a = _idct(ctx, small, np.full(64, 2, np.uint16))
    big = np.concatenate([small, np.full((1, 64), 3000)])
    assert ck.block_l1(small, np.full(64, 2)) <= L1_LIMIT < ck.block_l1(big, np.full(64, 2))
    assert np.array_equal(_idct(ctx, big, np.full(64, 2, np.uint16))[:33], a)


def test_idct_refusals(ctx):
    coef, qt, out = np.zeros((1, 64), np.int16), np.ones(64, np.uint16), np.zeros(64, np.uint8)
    f = ctx.lib.srl_jpeg_idct_blocks
    assert f(ctx.h, None, 1, capi._ptr(qt), capi._ptr(out)) == SRL_ERR_BAD_ARG and f(ctx.h, capi._ptr(coef), 1, None, capi._ptr(out)) == SRL_ERR_BAD_ARG
    assert f(ctx.h, capi._ptr(coef), 1, capi._ptr(qt), None) == SRL_ERR_BAD_ARG and f(ctx.h, capi._ptr(coef), 0, capi._ptr(qt), capi._ptr(out)) == SRL_ERR_BAD_ARG
    assert f(None, capi._ptr(coef), 1, capi._ptr(qt), capi._ptr(out)) == SRL_ERR_BAD_ARG


# ------------------------------------------------------------------------------------------------ 3. into the preparer
def _opts(rows, cols):
    return capi.default_image_prep_opts(rows=rows, cols=cols, fx=0.9 * cols, fy=0.92 * cols, cx=cols / 2 - 0.37, cy=rows / 2 + 0.21,
                                        dist=[0.2, 0.05, 0.002, -0.003, 0.01])


def _all_bytes(prep, tiles):
    stages = [prep.download_resized()] + [prep.download_stage(s, tiles) for s in range(5)] + [prep.download(0), prep.download(1)]
    return tuple(a.tobytes() for a in stages)


@pytest.mark.parametrize("name,size", [("40x48_420_rrow", (48, 40)), ("37x43_422_r2", (43, 37)), ("40x48_444_noise", (24, 20)), ("37x43_420_r1", (21, 18)),
                                       ("40x48_gray_r2", (17, 23))])
def test_prepare_jpeg_equals_the_prepare_of_the_downloaded_frame(name, size):
    """a preparer of the frame's size (srl_image_prepare's path), of exactly half of it (the box mean) and of other sizes (the general
    resize): every stage and both results are bytewise what the raw entry points give for the frame srl_jpeg_download returns"""
    data = GOLDEN[name][0]
    a, b = srl.Context(0), srl.Context(0)
    try:
        pa, pb = srl.ImagePrep(a, _opts(*size)), srl.ImagePrep(b, _opts(*size))
        ia = pa.prepare_jpeg(data)
        info = capi.jpeg_parse(data)
        frame = a.jpeg_download(info.rows, info.cols)
        _same(name, frame, GOLDEN[name][1])
        ib = pb.prepare(frame) if size == (info.rows, info.cols) else pb.prepare_resized(frame)
        assert ia.as_tuple() == ib.as_tuple()
        assert _all_bytes(pa, ia.tiles) == _all_bytes(pb, ib.tiles)
        # again, and with a raw frame in between: the same bytes
        first = _all_bytes(pa, ia.tiles)
        pa.prepare_resized(np.zeros((30, 31, 3), np.uint8))
        assert _all_bytes(pa, ia.tiles) != first
        pa.prepare_jpeg(data)
        assert _all_bytes(pa, ia.tiles) == first
    finally:
        a.close()
        b.close()


def test_the_flow_tracks_on_frames_that_came_compressed():
    names = ("40x48_420_rrow", "40x48_444_noise")
    pts = np.array([[12.0, 14.0], [20.5, 30.25], [30.0, 40.0], [5.0, 5.0]], np.float32)
    a, b = srl.Context(0), srl.Context(0)
    try:
        pa, pb = srl.ImagePrep(a, _opts(48, 40)), srl.ImagePrep(b, _opts(48, 40))
        fa, fb = srl.Flow(a), srl.Flow(b)
        for name in names:
            pa.prepare_jpeg(GOLDEN[name][0])
            pb.prepare(GOLDEN[name][1])
            ra, rb = fa.track_prepared(pts), fb.track_prepared(pts)
            assert ra[0].tobytes() == rb[0].tobytes() and ra[1].tobytes() == rb[1].tobytes() and ra[2] == rb[2]
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals_leave_the_previous_frame_and_the_prepared_images():
    ctx = srl.Context(0)
    try:
        lib = ctx.lib
        good_name = "37x43_420_r1"
        good = np.frombuffer(GOLDEN[good_name][0], np.uint8)
        out = np.zeros((43, 37, 3), np.uint8)
        assert lib.srl_jpeg_download(ctx.h, capi._ptr(out), out.strides[0]) == SRL_ERR_NO_SWEEP            # before any decode
        pinfo, jinfo = capi.ImagePrepInfo(), capi.JpegInfo()
        assert lib.srl_image_prepare_jpeg(ctx.h, capi._ptr(good), good.size, C.byref(pinfo)) == SRL_ERR_NO_MAP      # no preparer
        assert lib.srl_jpeg_download(ctx.h, capi._ptr(out), out.strides[0]) == SRL_ERR_NO_SWEEP            # ... and the stream was not decoded
        prep = srl.ImagePrep(ctx, _opts(43, 37))
        done = prep.prepare_jpeg(good)
        before = _all_bytes(prep, done.tiles)
        frame = ctx.jpeg_download(43, 37).tobytes()
        unsupported = bytearray(good); unsupported[unsupported.index(b"\xFF\xC0") + 1] = 0xC2              # a progressive frame header
        off = ck.parse(bytes(good))["scan_offset"]
        wrong_marker = bytearray(good); wrong_marker[wrong_marker.index(b"\xFF\xD0", off) + 1] = 0xD3
        streams = [(bytes(unsupported), SRL_ERR_UNSUPPORTED), (bytes(wrong_marker), SRL_ERR_BAD_ARG), (bytes(good[:off + 40]), SRL_ERR_BAD_ARG),
                   (bytes(good[:50]), SRL_ERR_BAD_ARG), (b"\x00\x01\x02\x03", SRL_ERR_BAD_ARG)]
        for data, status in streams:
            d = np.frombuffer(data, np.uint8)
            C.memset(C.byref(jinfo), 0xFF, C.sizeof(jinfo)); C.memset(C.byref(pinfo), 0xFF, C.sizeof(pinfo))
            assert lib.srl_jpeg_decode(ctx.h, capi._ptr(d), d.size, C.byref(jinfo)) == status and bytes(jinfo) == bytes(C.sizeof(jinfo))
            assert lib.srl_image_prepare_jpeg(ctx.h, capi._ptr(d), d.size, C.byref(pinfo)) == status and pinfo.as_tuple() == (0,) * 8
            assert ctx.jpeg_download(43, 37).tobytes() == frame
        assert lib.srl_jpeg_decode(ctx.h, None, 10, None) == SRL_ERR_BAD_ARG and lib.srl_jpeg_decode(ctx.h, capi._ptr(good), 1, None) == SRL_ERR_BAD_ARG
        assert lib.srl_jpeg_decode(None, capi._ptr(good), good.size, None) == SRL_ERR_BAD_ARG
        assert lib.srl_jpeg_download(ctx.h, None, 3 * 37) == SRL_ERR_BAD_ARG and lib.srl_jpeg_download(ctx.h, capi._ptr(out), 3 * 37 - 1) == SRL_ERR_BAD_ARG
        ctx.comm_set_host_callbacks(2, 0, lambda a: None, lambda v: [v, v])                                # more than one rank
        assert lib.srl_jpeg_decode(ctx.h, capi._ptr(good), good.size, C.byref(jinfo)) == SRL_ERR_UNSUPPORTED and jinfo.rows == 0
        assert lib.srl_image_prepare_jpeg(ctx.h, capi._ptr(good), good.size, C.byref(pinfo)) == SRL_ERR_UNSUPPORTED
        ctx.comm_set_host_callbacks(1, 0, None, None)
        assert ctx.jpeg_download(43, 37).tobytes() == frame and _all_bytes(prep, done.tiles) == before
        # a larger frame grows the decoder's blocks (the frame the preparer's chain read is gone with them: the read-back says so) ...
        ctx.jpeg_decode(GOLDEN["40x48_444_noise"][0])
        resized = np.zeros((43, 37, 3), np.uint8)
        assert lib.srl_image_prep_download_resized(ctx.h, capi._ptr(resized), resized.size) == SRL_ERR_NO_SWEEP
        assert prep.download(0).tobytes() == before[6]
        # ... and everything still works
        assert _all_bytes(prep, prep.prepare_jpeg(good).tiles) == before
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------ 5. the mirror
def test_image_process_jpeg_equals_image_process_of_the_decoded_frame():
    """two frames through srl_lio_image_process_jpeg on one handle and, decoded first (srl_jpeg_decode + srl_jpeg_download), through
    srl_lio_image_process on another: the same result records, camera state, covariance and pose maps"""
    pytest.importorskip("PIL")                             # the frames of tests/test_gpu_image_process.py, compressed here
    import test_gpu_image_process as ip
    frames = ip._frames(ip.ROWS, ip.COLS, 2)
    a, b = ip._lio(ip.COLS, ip.ROWS, 1.0, 40.0, 300), ip._lio(ip.COLS, ip.ROWS, 1.0, 40.0, 300)
    try:
        for k, raw in enumerate(frames):
            data = jc.encode(np.ascontiguousarray(raw[:, :, ::-1]), "420", quality=90)
            info = b.ctx.jpeg_decode(data)
            assert (info.rows, info.cols) == (ip.ROWS, ip.COLS)
            decoded = b.ctx.jpeg_download(info.rows, info.cols)
            assert np.array_equal(decoded, jc.pillow_decode(data))
            ra = a.image_process_jpeg(data, ip.T0 + ip.DT * k, k + 1)
            rb = b.image_process(decoded, ip.T0 + ip.DT * k, k + 1)
            assert bytes(ra) == bytes(rb) and ra.first_data == int(k == 0) and (ra.prepared_rows, ra.prepared_cols) == (ip.ROWS, ip.COLS)
            assert a.vio_get_camera_state().tobytes() == b.vio_get_camera_state().tobytes() and a.vio_get_cov().tobytes() == b.vio_get_cov().tobytes()
            oa, ob = a.image_oft(), b.image_oft()
            assert all(oa.pose_map(w).tobytes() == ob.pose_map(w).tobytes() for w in (0, 1)) and oa.sizes() == ob.sizes()
            assert a.image_time_last_process() == b.image_time_last_process() == ip.T0 + ip.DT * k
        assert ra.tracked_after_flow >= 30                 # the second frame did track: the comparison is not of two idle frames
    finally:
        a.close()
        b.close()
