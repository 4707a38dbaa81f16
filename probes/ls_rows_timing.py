#!/usr/bin/env python3
"""Does a change of the HOST paths of the least-squares rows (runtime.py, irl.py) cost host time per evaluation?  Two copies of the package in one process - the working
tree's and another checkout's (--parent: the package directory of the commit to compare with, built) - on the same data, alternating inside every round:

    batched         BatchedLMLoop.for_sysid(...).step(): one evaluation launch and one update launch per step, nothing read back - quadrotor SysID, K = 1024 problems of
                    S = 1 trajectory, T = 100 (the shape of probes/lm_batched_timing.py); HIP events around --steps back-to-back steps behind 20 warm-up steps
    batched_wls     the same with weights (pdp_sysid_step_wls_batched)
    evaluate        LMLoop.for_sysid at B = 1024, T = 100: the evaluation call alone, a host clock around --calls calls, each ended by its own one copy to the host
    evaluate_wls    the same with weights

The kernels of the two copies are the same code objects (probes/code_object_diff.py says so for a host-only change), so what can differ is the time the host needs to
issue them.  Reported per variant and copy: median over --rounds rounds, min and max.  Criterion: the tree's median may exceed the other copy's median by no more than that
copy's own min-to-max spread in this run.  Exit status 1 where it does.

    python probes/ls_rows_timing.py --parent <other checkout>/pontryagin-differentiable-programming_amd [--out profiles/ls_rows_timing.txt]
"""
import argparse
import importlib
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_package(path, name):
    """the package directory `path` imported under `name` (its modules import each other relatively)"""
    spec = importlib.util.spec_from_file_location(name, os.path.join(path, "__init__.py"), submodule_search_locations=[path])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return {k: importlib.import_module("%s.%s" % (name, k)) for k in ("runtime", "zoo", "irl")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--problems", type=int, default=1024)
    ap.add_argument("--horizon", type=int, default=100)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    copies = {"parent": load_package(os.path.abspath(a.parent), "pdp_amd_parent"), "tree": load_package(os.path.join(ROOT, "pontryagin-differentiable-programming_amd"), "pdp_amd")}
    K, T = a.problems, a.horizon
    io = np.load(os.path.join(ROOT, "tests", "golden", "iodata_quadrotor.npz"))
    rng = np.random.default_rng(0)
    n, p = io["states"].shape[2], io["true_parameter"].size
    x0 = io["states"][np.arange(K) % io["states"].shape[0], 0] * (1.0 + 0.05 * rng.standard_normal((K, n)))
    u = rng.uniform(-1.0, 1.0, (K, T, io["inputs"].shape[2]))
    theta0 = io["true_parameter"][None] * (1.0 + 0.05 * rng.standard_normal((K, p)))
    weights = 1.0 / (0.5 + np.arange(n)) ** 2
    runs = {}
    for who, pk in copies.items():
        rt, mdl = pk["runtime"], pk["zoo"].get("quadrotor", "sysid")
        u_d = rt.dev(u)
        xobs = mdl.sysid_integrate(rt.dev(x0), u_d, io["true_parameter"])          # the data: rolled out at the true parameter
        for tag, kw in (("", {}), ("_wls", dict(weights=weights))):
            # max_evals beyond every window: no problem ends by its budget inside one
            batched = pk["irl"].BatchedLMLoop.for_sysid(mdl, u_d, xobs, theta0, max_evals=1 << 30, trace_len=4, **kw)
            single = pk["irl"].LMLoop.for_sysid(mdl, u_d, xobs, theta0[0], **kw)
            runs["batched" + tag, who] = ("events", batched.step)
            runs["evaluate" + tag, who] = ("clock", lambda f=single.evaluate, th=theta0[0].copy(): f(th))
    variants = ("batched", "batched_wls", "evaluate", "evaluate_wls")
    times = {k: [] for k in runs}
    for r in range(a.rounds + 1):
        for v in variants:
            for who in ("parent", "tree") if r % 2 else ("tree", "parent"):
                how, f = runs[v, who]
                if how == "events":
                    for _ in range(20):
                        f()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.steps):
                        f()
                    e1.record()
                    e1.synchronize()
                    ms = e0.elapsed_time(e1) / a.steps
                else:
                    for _ in range(5):
                        f()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        assert f() is not None
                    ms = 1e3 * (time.perf_counter() - t0) / a.calls
                if r > 0:                                            # round 0 is warm-up as a whole
                    times[v, who].append(ms)
    lines = ["Host paths of the least-squares rows, the working tree's package against the --parent package; quadrotor SysID, K = B = %d, T = %d; %s"
             % (K, T, torch.cuda.get_device_name(0)),
             "ms per step / per call: batched* = HIP events around %d back-to-back BatchedLMLoop.step() behind 20 warm-up steps; evaluate* = host clock around %d "
             "LMLoop evaluations, each ended by its copy to the host; the copies alternate, %d rounds" % (a.steps, a.calls, a.rounds),
             "criterion: median(tree) <= median(parent) + (max(parent) - min(parent))"]
    ok = True
    for v in variants:
        tp, tt = np.array(times[v, "parent"]), np.array(times[v, "tree"])
        bound = float(np.median(tp) + tp.max() - tp.min())
        good = float(np.median(tt)) <= bound
        ok = ok and good
        lines.append("  %-13s parent median %.4f  min %.4f  max %.4f   tree median %.4f  min %.4f  max %.4f   tree / parent %.3f   bound %.4f  %s"
                     % (v, np.median(tp), tp.min(), tp.max(), np.median(tt), tt.min(), tt.max(), np.median(tt) / np.median(tp), bound, "ok" if good else "EXCEEDED"))
    txt = "\n".join(lines) + "\n"
    print(txt, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(txt)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
