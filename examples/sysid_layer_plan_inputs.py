#!/usr/bin/env python3
"""Planning inputs THROUGH an identified model, with the SysID rollout as a torch.autograd layer that is differentiable in its inputs.

Once a model has been identified (examples/sysid_pdp.py, examples/sysid_layer_custom_loss.py) its rollout is a differentiable simulator: here the pendulum's SysID
model at its true parameter (length, mass, damping) is held fixed - theta requires no gradient, and none is computed - and torch's Adam moves the INPUTS of 16 rollouts
from 16 initial states so that the pendulum ends upright and at rest, JinEnv.SinglePendulum's goal [pi, 0], with a small price on effort.  The loss is written in torch
on the output of pdp_amd.autograd.sysid_trajectory(..., input_grad=True); `loss.backward()` gives dL/dinputs through the dynamics from one launch of the adjoint sweep
(dL/du_t = G_t' lam_{t+1}, include/pdp_hip_sysid_vjp_u.h), and torch adds the effort term's own gradient.

    python examples/sysid_layer_plan_inputs.py --iters 300 --lr 5e-2
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pdp_amd import PDP, zoo                        # noqa: E402
from pdp_amd.autograd import sysid_trajectory       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--lr", type=float, default=5e-2)
    ap.add_argument("--batch", type=int, default=16, help="number of initial states")
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--effort", type=float, default=1e-3, help="weight of the mean squared input")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    env, dt = zoo.make_env("pendulum", "sysid")
    sid = PDP.SysID("pendulum")
    sid.setAuxvarVariable(env.dyn_auxvar)
    sid.setStateVariable(env.X)
    sid.setControlVariable(env.U)
    sid.setDyn(env.X + dt * env.f)

    rng = np.random.default_rng(a.seed)
    B, T = a.batch, a.horizon
    theta = torch.tensor([1.0, 1.0, 0.05], dtype=torch.float64, device="cuda")       # l, m, damping_ratio: the identified model, held fixed
    x0 = torch.as_tensor(np.stack([rng.uniform(-1.0, 1.0, B), rng.uniform(-1.0, 1.0, B)], axis=1), device="cuda")
    goal = torch.tensor([math.pi, 0.0], dtype=torch.float64, device="cuda")
    inputs = torch.zeros((B, T, 1), dtype=torch.float64, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([inputs], lr=a.lr)

    def evaluate():
        state = sysid_trajectory(sid, x0, inputs, theta, input_grad=True)
        miss = ((state[:, -1] - goal) ** 2).sum(dim=1)
        return miss.mean() + a.effort * (inputs ** 2).mean(), float(miss.detach().max().sqrt())

    with torch.no_grad():
        first, miss = evaluate()
    print("initial: loss %.6e  largest distance from the goal %.4e" % (float(first), miss))
    t0 = time.time()
    for k in range(a.iters):
        opt.zero_grad()
        loss, miss = evaluate()
        loss.backward()
        opt.step()
        if k % 50 == 0:
            print("iter %5d  loss %.6e  largest distance from the goal %.4e  largest |input| %.3f" % (k, float(loss.detach()), miss, float(inputs.detach().abs().max())))
    elapsed = time.time() - t0
    with torch.no_grad():
        last, miss = evaluate()
    print("final:   loss %.6e  largest distance from the goal %.4e" % (float(last), miss))
    print("done: %d iterations x %d rollouts of %d steps in %.2f s" % (a.iters, B, T, elapsed))
    return float(first), float(last)


if __name__ == "__main__":
    main()
