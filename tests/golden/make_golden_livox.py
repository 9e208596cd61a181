"""Writes tests/golden/golden_livox.npz: what the reference's own cloudProcessing::livoxHandler (tests/livox_ref_reader.cpp, compiled into a
temporary directory with src/cloudProcessing.cpp where it lies) queues for the tie-free cases of tests/livox_cases.py that have a valid
point -- so that a machine without the reference tree can hold the device decode against the reference.  Data only.  Per case `name`:
name/count, name/last_end_time, and name/records ((count, 5): raw_point, relative_time, timestamp) or, beyond
livox_reader.GOLDEN_FULL_RECORDS records, name/sha256 of those bytes with the first and last record as name/ends.
Run from the repository root: python tests/golden/make_golden_livox.py"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import livox_cases as lc  # noqa: E402
import livox_reader as lr  # noqa: E402

if __name__ == "__main__":
    pack, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        reader = lr.build(tmp)
        for c in lc.reference_cases():
            if c["name"] in lc.UNDEFINED_UPSTREAM:
                continue
            rows, last_end = lr.run(reader, c)
            rec = lr.records_of(rows)
            names.append(c["name"])
            pack[c["name"] + "/count"] = np.int64(len(rec))
            pack[c["name"] + "/last_end_time"] = np.float64(last_end)
            if len(rec) <= lr.GOLDEN_FULL_RECORDS:
                pack[c["name"] + "/records"] = rec
            else:
                pack[c["name"] + "/sha256"] = lr.digest(rec)
                pack[c["name"] + "/ends"] = rec[[0, -1]]
    pack["names"] = np.array(names)
    out = os.path.join(HERE, "golden_livox.npz")
    np.savez_compressed(out, **pack)
    print(out, os.path.getsize(out), "bytes")
