#!/usr/bin/env python3
"""Identifying a pendulum from a NONLINEAR OBSERVATION, with the SysID rollout as a torch.autograd layer.

The reference's SysID drivers (Examples/SysID/<sys>/*_PDP.py) hard-wire one loss: the squared distance between the rollout and the recorded STATES.  Here the state is
never recorded: a camera sees the direction of the rod, (sin q, cos q), at every step - no angular velocity, and the angle itself only up to full turns.  The loss is
written in torch on the output of pdp_amd.autograd.sysid_trajectory, `loss.backward()` differentiates through the rollout (one launch of the adjoint sweep,
include/pdp_hip_sysid_vjp.h), and a torch.optim optimiser moves the three parameters (length, mass, damping) together with the unknown initial velocity of every
recording, which is a component of the layer's ini_state.

The recordings are generated here: rollouts at the true parameter from a fixed seed (SysID.integrateDyn_batch).

    python examples/sysid_layer_custom_loss.py --iters 400 --lr 2e-2
"""
import argparse
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
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--lr", type=float, default=2e-2)
    ap.add_argument("--batch", type=int, default=16, help="number of recordings")
    ap.add_argument("--horizon", type=int, default=40)
    ap.add_argument("--sigma", type=float, default=0.4, help="initial parameter = true (1 + U(-sigma/2, sigma/2))")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()

    env, dt = zoo.make_env("pendulum", "sysid")
    sid = PDP.SysID("pendulum")
    sid.setAuxvarVariable(env.dyn_auxvar)
    sid.setStateVariable(env.X)
    sid.setControlVariable(env.U)
    sid.setDyn(env.X + dt * env.f)

    rng = np.random.default_rng(a.seed)
    true_parameter = np.array([1.0, 1.0, 0.05])                                     # l, m, damping_ratio
    B, T = a.batch, a.horizon
    inputs = torch.as_tensor(rng.uniform(-4.0, 4.0, (B, T, 1)), device="cuda")
    x0_true = np.stack([rng.uniform(-1.0, 1.0, B), rng.uniform(-1.0, 1.0, B)], axis=1)
    recorded = sid.integrateDyn_batch(x0_true, inputs, true_parameter)              # [B, T+1, 2] - of which only the direction of the rod is kept
    seen = torch.stack([torch.sin(recorded[:, :, 0]), torch.cos(recorded[:, :, 0])], dim=2)
    q0 = torch.atan2(seen[:, 0, 0], seen[:, 0, 1])                                  # the initial angle is seen; the initial velocity is not
    del recorded

    theta = torch.tensor(true_parameter * (1.0 + a.sigma * rng.random(3) - a.sigma / 2), dtype=torch.float64, device="cuda", requires_grad=True)
    dq0 = torch.zeros(B, dtype=torch.float64, device="cuda", requires_grad=True)
    opt = torch.optim.Adam([theta, dq0], lr=a.lr)

    def errors():
        return (float(np.abs(theta.detach().cpu().numpy() - true_parameter).max()), float(np.abs(dq0.detach().cpu().numpy() - x0_true[:, 1]).max()))

    def evaluate():
        state = sysid_trajectory(sid, torch.stack([q0, dq0], dim=1), inputs, theta)
        q = state[:, :, 0]
        return ((torch.sin(q) - seen[:, :, 0]) ** 2 + (torch.cos(q) - seen[:, :, 1]) ** 2).mean()

    with torch.no_grad():
        first = float(evaluate())
    print("initial: loss %.6e  parameter error %.4e  initial-velocity error %.4e" % ((first,) + errors()))
    t0 = time.time()
    for k in range(a.iters):
        opt.zero_grad()
        loss = evaluate()
        loss.backward()
        opt.step()
        if k % 50 == 0:
            print("iter %5d  loss %.6e  |theta - theta*| %.4e  |dq0 - dq0*| %.4e" % ((k, float(loss.detach())) + errors()))
    elapsed = time.time() - t0
    with torch.no_grad():
        last = float(evaluate())
    print("final:   loss %.6e  parameter error %.4e  initial-velocity error %.4e" % ((last,) + errors()))
    print("done: %d iterations x %d recordings of %d steps in %.2f s" % (a.iters, B, T, elapsed))
    return first, last


if __name__ == "__main__":
    main()
