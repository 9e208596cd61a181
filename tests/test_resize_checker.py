"""The resize of the image preparation without a device (CPU): srl_image_resize_build_tables (pure host code) against the tables of
tests/resize_checker.py, bytewise; the properties the specification promises of the tables; and the checker's own pixel rule against
FP64 bilinear interpolation at the same sample positions, on the shapes that tests/test_gpu_image_resize.py runs on the device.

The bound of 1.5 grey levels is the sum of what the fixed-point rule may lose, with room to spare: the two rounded coefficient pairs
2 x 255 x 0.5 / 2048 = 0.12, the two `>> 16` truncations (each below one unit of the 2-bit fraction that is left: under 0.5 together), the
`>> 4` truncations (under 1 / 128), the final rounding 0.5, and the FP32 sample position (below 0.01 at these sizes)."""
import ctypes as C

import numpy as np
import pytest

import resize_cases as rc
import resize_checker as rk
import sr_livo_amd as srl
from sr_livo_amd import capi

SRL_OK, SRL_ERR_BAD_ARG = 0, -3
LENGTHS = [(1, 1), (1, 5), (5, 1), (53, 53), (106, 53), (91, 53), (27, 53), (340, 170), (341, 170)]


@pytest.mark.parametrize("src,dst", LENGTHS)
def test_the_library_builds_the_checkers_tables(src, dst):
    ofs, coef = srl.image_resize_build_tables(src, dst)
    wofs, wcoef = rk.build_tables(src, dst)
    assert ofs.dtype == wofs.dtype == np.int32 and coef.dtype == wcoef.dtype == np.int16
    assert ofs.shape == (dst,) and coef.shape == (dst, 2)
    assert ofs.tobytes() == wofs.tobytes() and coef.tobytes() == wcoef.tobytes(), (ofs, wofs, coef, wcoef)


@pytest.mark.parametrize("src,dst", LENGTHS)
def test_table_properties(src, dst):
    ofs, coef = srl.image_resize_build_tables(src, dst)
    total = coef.astype(np.int64).sum(axis=1)
    assert (coef >= 0).all() and (total >= 2047).all() and (total <= 2049).all()
    assert (np.diff(ofs) >= 0).all() and ofs.min() >= 0 and ofs.max() <= src - 1
    assert (coef[ofs == src - 1, 1] == 0).all()          # the clamped last tap carries no weight
    if src == dst:
        assert np.array_equal(ofs, np.arange(dst)) and (coef[:, 0] == 2048).all() and (coef[:, 1] == 0).all()


def test_known_tables():
    # 5 -> 3: positions 1/3, 2, 3 + 2/3; 2048 / 3 = 682.67 and 1365.33
    ofs, coef = srl.image_resize_build_tables(5, 3)
    assert ofs.tolist() == [0, 2, 3] and coef.tolist() == [[1365, 683], [2048, 0], [683, 1365]]
    # 2 -> 4: positions -0.25 (clamped below), 0.25, 0.75, 1.25 (clamped above)
    ofs, coef = srl.image_resize_build_tables(2, 4)
    assert ofs.tolist() == [0, 0, 0, 1] and coef.tolist() == [[2048, 0], [1536, 512], [512, 1536], [2048, 0]]
    # exactly half: every position d * 2 + 0.5
    ofs, coef = srl.image_resize_build_tables(8, 4)
    assert ofs.tolist() == [0, 2, 4, 6] and (coef == 1024).all()


def test_the_builder_refuses_without_touching_the_arrays():
    lib = srl.load_library()
    ofs = np.full(4, 7, np.int32)
    coef = np.full((4, 2), 7, np.int16)
    for src, dst in ((0, 4), (-1, 4), (4, 0), (4, -3)):
        assert lib.srl_image_resize_build_tables(src, dst, capi._ptr(ofs), capi._ptr(coef)) == SRL_ERR_BAD_ARG
    assert lib.srl_image_resize_build_tables(4, 4, None, capi._ptr(coef)) == SRL_ERR_BAD_ARG
    assert lib.srl_image_resize_build_tables(4, 4, capi._ptr(ofs), None) == SRL_ERR_BAD_ARG
    assert (ofs == 7).all() and (coef == 7).all()
    assert lib.srl_image_resize_build_tables(4, 4, capi._ptr(ofs), capi._ptr(coef)) == SRL_OK and ofs.tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("src,dst,what", rc.SHAPES, ids=[s[2] for s in rc.SHAPES])
def test_the_checker_stays_within_the_fixed_point_error_of_fp64_bilinear(src, dst, what):
    img = np.ascontiguousarray(rc.image(src[0], src[1], 31))
    got = rk.linear(img, dst[0], dst[1]).astype(np.float64)
    want = rk.bilinear_fp64(img, dst[0], dst[1])
    err = float(np.abs(got - want).max())
    print(f"{src} -> {dst}: max |fixed point - FP64 bilinear| = {err:.4f} grey levels")
    assert err < 1.5, err
    if src == (1, 1):
        assert (got == img[0, 0]).all()


def test_exact_half_is_the_box_mean():
    src, dst = rc.SHAPES[0][0], rc.SHAPES[0][1]
    img = np.ascontiguousarray(rc.image(src[0], src[1], 31))
    assert rk.is_exact_half(img.shape, dst[0], dst[1]) and not rk.is_exact_half((193, 341), 96, 170) and not rk.is_exact_half((74, 105), 37, 53)
    got = rk.resize(img, dst[0], dst[1])
    s = img.astype(np.int64)
    want = np.zeros((dst[0], dst[1], 3), np.int64)
    for i in range(dst[0]):                              # the definition, pixel by pixel
        for j in range(dst[1]):
            want[i, j] = (s[2 * i, 2 * j] + s[2 * i, 2 * j + 1] + s[2 * i + 1, 2 * j] + s[2 * i + 1, 2 * j + 1] + 2) >> 2
    assert np.array_equal(got, want)
    # ... and the general rule agrees here: with every coefficient 1024 its shifts drop only zeros (h = 1024 (s0 + s1), a multiple of 16;
    # 1024 (h >> 4) = 65536 (s0 + s1)), so it ends in the same (sum + 2) >> 2
    assert np.array_equal(got, rk.linear(img, dst[0], dst[1]))
    # equal sizes: the image itself
    assert np.array_equal(rk.resize(img, src[0], src[1]), img)


def test_entries_refuse_a_null_context_and_zero_the_info():
    lib = srl.load_library()
    for s in ("srl_image_resize_build_tables", "srl_image_prepare_resized", "srl_image_prep_download_resized"):
        assert s in srl.declared_symbols() and s in srl.library_symbols(), s
    img = np.zeros((48, 64, 3), np.uint8)
    out = np.full((48, 64, 3), 7, np.uint8)
    info = capi.ImagePrepInfo()
    C.memset(C.byref(info), 0xFF, C.sizeof(info))
    assert lib.srl_image_prepare_resized(None, capi._ptr(img), 48, 64, 192, C.byref(info)) == SRL_ERR_BAD_ARG
    assert bytes(info) == bytes(C.sizeof(info))
    assert lib.srl_image_prepare_resized(None, None, 48, 64, 192, None) == SRL_ERR_BAD_ARG
    assert lib.srl_image_prep_download_resized(None, capi._ptr(out), out.size) == SRL_ERR_BAD_ARG and (out == 7).all()
