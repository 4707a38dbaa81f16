"""Writes tests/golden/fused3_sched_parent.npz: the outputs of every case of tests/fused3_sched_common.py on the build of the checkout it is run from (GPU).
Run it from a checkout of the commit whose bits are to be kept - for tests/test_gpu_fused3_sched.py the parent of the commit that scheduled the runner's steps:

    python probes/record_fused3_sched_golden.py <commit hash> <output.npz>

The hash is stored in the file as given (a checkout copied without its .git directory cannot name its own commit)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fused3_sched_common as fc      # noqa: E402

commit, path = sys.argv[1], sys.argv[2]
rec = {"seed": np.int64(fc.SEED), "commit": np.array(commit)}
t5 = None
for name in fc.CASES:
    out = fc.run_case(name, given=t5)
    if name == "T5":
        t5 = (out["x"], out["lam"])
    for k, v in out.items():
        rec["%s/%s" % (name, k)] = v
    print(name, {k: v.shape for k, v in out.items()}, "status", out["status"].tolist())
os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
np.savez_compressed(path, **rec)
print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
