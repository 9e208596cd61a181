"""A measurement with its camera frame given compressed (srl_lio_run_measurement_image_jpeg) against the same measurement with the frame
decoded first (srl_jpeg_decode + srl_jpeg_download) and handed to srl_lio_run_measurement_image: the sequence, the handles and the
snapshot are those of tests/test_gpu_run_measurement_image.py; every part of the snapshot -- state, filter, camera state and covariance,
pose maps, candidates, the colour map's colours, the map -- agrees bytewise behind each processed frame.  The two replays run one after
the other (the initial flag and g_norm are the process's, as in that file)."""
import numpy as np
import pytest

import jpeg_cases as jc
import test_gpu_run_measurement_image as rm

pytestmark = pytest.mark.gpu
FRAMES = 2


def _replay(streams, compressed):
    lio, out = rm._lio(True), []
    try:
        for k, ms in enumerate(rm._sequence()):
            if compressed:
                r = lio.run_measurement_image_jpeg(*rm._args(ms), streams[k])
            else:
                info = lio.ctx.jpeg_decode(streams[k])
                r = lio.run_measurement_image(*rm._args(ms), lio.ctx.jpeg_download(info.rows, info.cols))
            assert r["rc"] == 0
            if not r["processed"]:
                assert bytes(r["image"]) == bytes(len(bytes(r["image"])))      # no camera frame while the filter initialises
                continue
            out.append((k, rm._snapshot(lio, r, r["image"]), (r["image"].prepared_rows, r["image"].prepared_cols)))
            if len(out) == FRAMES:
                # no image: exactly the measurement
                r = lio.run_measurement_image_jpeg(*rm._args(rm._sequence()[k + 1]), None)
                assert r["rc"] == 0 and bytes(r["image"]) == bytes(len(bytes(r["image"])))
                break
        return out
    finally:
        lio.set_initial_flag(False)
        lio.close()


def test_the_compressed_frame_gives_what_the_decoded_frame_gives():
    pytest.importorskip("PIL")                             # the sequence's frames, compressed here
    streams = [jc.encode(np.ascontiguousarray(rm._image(k)[:, :, ::-1]), "420", quality=90) for k in range(len(rm._sequence()))]
    got, want = _replay(streams, True), _replay(streams, False)
    assert len(got) == len(want) == FRAMES
    for (ka, sa, size_a), (kb, sb, size_b) in zip(got, want):
        assert ka == kb and size_a == size_b == (rm.ROWS, rm.COLS)
        for name in sa:
            assert sa[name] == sb[name], (ka, name)
