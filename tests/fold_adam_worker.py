"""The unfused reference of tests/test_fold_adam_gpu.py: every case of tests/fold_adam_cases.py with TN_FOLD_ADAM=0 in a process of its own (the
library reads the switch once per process), records saved with torch.save.

    TN_FOLD_ADAM=0 python tests/fold_adam_worker.py <golden_dir> <out.pt>
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    assert os.environ.get("TN_FOLD_ADAM") == "0", "the worker is the unfused path"
    from fold_adam_cases import CASES, run_case

    golden_dir, out = sys.argv[1], sys.argv[2]
    records = {}
    for name in CASES:
        recs = run_case(name, golden_dir)
        for r in recs:
            del r["pre"]  # (the test takes its own)
        records[name] = recs
    torch.save(records, out)


if __name__ == "__main__":
    main()
