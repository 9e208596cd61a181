"""What tests/test_gpu_image_prep.py and tests/test_gpu_image_prep_envelope.py share: the bytewise comparison of a preparer's stages, results
and info record with the dict of tests/imgprep_checker.py's prepare()."""
import numpy as np

from sr_livo_amd import capi


def same(name, got, want):
    want = np.ascontiguousarray(want)
    assert got.size == want.size, (name, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, (name, bad.size, bad[:8], got.ravel()[bad[:8]], want.ravel()[bad[:8]])


def check_all(prep, info, want, installed=0):
    assert info.as_tuple() == want["info"] + (installed,), (info.as_tuple(), want["info"])
    T = info.tiles
    same("undist", prep.download_stage(capi.SRL_PREP_STAGE_UNDIST, T), want["undist"])
    same("gray", prep.download_stage(capi.SRL_PREP_STAGE_GRAY, T), want["gray"])
    ycrcb = np.concatenate([want["y"].ravel(), np.stack([want["cr"], want["cb"]], axis=-1).ravel()])
    same("ycrcb", prep.download_stage(capi.SRL_PREP_STAGE_YCRCB, T), ycrcb)
    same("lut_gray", prep.download_stage(capi.SRL_PREP_STAGE_LUT_GRAY, T), want["lut_gray"])
    same("lut_y", prep.download_stage(capi.SRL_PREP_STAGE_LUT_Y, T), want["lut_y"])
    same("gray_eq", prep.download(capi.SRL_PREP_GRAY_EQ), want["gray_eq"])
    same("bgr_eq", prep.download(capi.SRL_PREP_BGR_EQ), want["bgr_eq"])


def all_bytes(prep, tiles):
    """every stage and both results as bytes, for comparing one run with another"""
    return tuple(prep.download_stage(s, tiles).tobytes() for s in range(5)) + (prep.download(0).tobytes(), prep.download(1).tobytes())
