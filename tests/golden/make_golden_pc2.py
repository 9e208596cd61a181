"""Writes tests/golden/golden_pc2.npz: what the reference's own cloudProcessing::process (tests/pc2_ref_reader.cpp, compiled into a temporary
directory with src/cloudProcessing.cpp where it lies) queues for the cases of tests/pc2_cases.py that are pinned to it -- so that a machine
without the reference tree can hold the device decode against the reference.  Data only.  Per case `name` and message k:
name/k/count, name/k/last_end_time and name/k/given (the class's members after the message; absent for an empty message), and
name/k/records ((count, 5): raw_point, relative_time, timestamp) or, beyond pc2_reader.GOLDEN_FULL_RECORDS records, name/k/sha256 of those
bytes with the first and last record as name/k/ends.  The tie-free cases keep the reference's order; the cases of
pc2_cases.MULTISET_CASES are stored sorted by relative_time, then by bytes (among equal keys the reference's order is its library's own).
Run from the repository root: python tests/golden/make_golden_pc2.py"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pc2_cases as pc  # noqa: E402
import pc2_reader as pr  # noqa: E402

if __name__ == "__main__":
    pack, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        reader = pr.build(tmp)
        for c in pc.exact_cases() + pc.multiset_cases():
            names.append(c["name"])
            for k, (rows, last_end, given) in enumerate(pr.run(reader, c)):
                key = f"{c['name']}/{k}"
                rec = pr.records_of(rows)
                if c["name"] in pc.MULTISET_CASES:
                    rec = np.array([np.frombuffer(b, dtype=np.float64) for _, b in sorted((float(r[3]), r.tobytes()) for r in rec)]).reshape(-1, 5)
                pack[key + "/count"] = np.int64(len(rec))
                if c["msgs"][k]["layout"].width * c["msgs"][k]["layout"].height > 0:
                    pack[key + "/last_end_time"] = np.float64(last_end)
                    pack[key + "/given"] = np.int64(given)
                if len(rec) <= pr.GOLDEN_FULL_RECORDS:
                    pack[key + "/records"] = rec
                else:
                    pack[key + "/sha256"] = pr.digest(rec)
                    pack[key + "/ends"] = rec[[0, -1]]
    pack["names"] = np.array(names)
    out = os.path.join(HERE, "golden_pc2.npz")
    np.savez_compressed(out, **pack)
    print(out, os.path.getsize(out), "bytes")
