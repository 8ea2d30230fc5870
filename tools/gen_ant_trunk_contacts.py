#!/usr/bin/env python
"""Record tests/golden/ant_mw_trunk_contacts.npz: the arrays tests/test_gpu_ant_trunk_contacts.py compares after every step, from the library this
tree loads (or MI_ENGINE_LIB), on the GPU.  The scenario -- env count, seeds, which envs are put on the ground -- is the test module's own.

Record it from the build whose results are to be kept, BEFORE an edit of the sub-step that must not change a bit, and commit it with that edit:

    python tools/gen_ant_trunk_contacts.py [--out tests/golden/ant_mw_trunk_contacts.npz]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ant_mw_trunk_contacts.npz"))
    args = ap.parse_args()
    import test_gpu_ant_trunk_contacts as scenario
    from isaacgymenvs_amd import native
    acts = scenario.actions()
    one = scenario.rollout(scenario.make_env(1), acts)
    sep = scenario.rollout(scenario.make_env(0), acts)
    for k in scenario.ARRAYS:
        assert np.array_equal(one[k], sep[k]), f"{k}: the one-launch form and the separate launches differ in the recording library"
    ci = one["contact_impulse"]
    for step in range(scenario.STEPS):
        assert (ci[step, :16, 0, 0] > 0).any() and (ci[step, 16:32, 0, 0] > 0).any(), f"step {step}: no torso contact recorded"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez_compressed(args.out, actions=acts, **one)
    print("recorded", args.out, os.path.getsize(args.out), "bytes, library", native.LIB_PATH)


if __name__ == "__main__":
    main()
