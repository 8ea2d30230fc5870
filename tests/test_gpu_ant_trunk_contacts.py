"""GPU test of the trunk-sphere rows of the Ant's limb-per-wave sub-step (csrc/core/engine_mw.hpp substep_role): the torso sphere and the four hip
stubs belong to the trunk role, and in a rollout they almost never touch the ground (the task ends an episode at a root height of 0.31, the torso
sphere has radius 0.25 and the contact offset is 0.02).  Here the root states are written before every step so that the three workgroups of 16 + 16 +
8 live lanes see the three cases the wave-uniform tests of these rows can meet: contact in some lanes, in every lane, in none.

The arrays after every step are compared between the one-launch form and one launch per sub-step plus the post kernel, and against a fixture recorded
with tools/gen_ant_trunk_contacts.py (both forms share substep_role, so only the fixture can see a change inside it).  The committed fixture was
recorded on an MI355X from the library of the commit before the sweep loop of substep_role was rearranged (profiles/ant_sweep_trunk_ab.txt)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, STEPS, SEED, ACTION_SEED = 40, 6, 7, 11
ARRAYS = ("obs", "rew", "reset", "root", "dof", "contact_impulse", "force_sensor")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ant_mw_trunk_contacts.npz")

LOW_Z = 0.24                                        # upright: torso sphere 0.01 into the ground (the legs, far deeper in, lift it again)
LOW_WG0 = (1, 2, 4, 7, 9, 10, 13)                   # workgroup 0: the lanes whose torso is put on the ground
LOW = LOW_WG0 + tuple(range(16, 32))                # workgroup 1: every lane; workgroup 2 (envs 32 .. 39): none
# on their back (half a turn about x), legs in the air, the torso sphere touching the ground and coming down: these carry their weight on it
FLIPPED = (2, 7, 9, 10, 17, 18, 20, 23, 26, 27, 29, 30)
FLIPPED_Z, FLIPPED_VZ = 0.25, -0.3
ROLLED = (4, 13, 22, 25)                            # on their back and rolled on by 50 degrees (230 about x): a hip stub comes within the contact offset as well
# An env below the termination height at step k is flagged by that step's post step and reset (root, dofs, impulses cleared) by the post step of
# step k + 1.  The odd envs start with their reset flag set, so that after every step one half of the flipped envs holds this step's impulses and
# the other half zeros.
FLAGGED_AT_START = tuple(e for e in LOW if e % 2)


def actions():
    return (np.random.default_rng(ACTION_SEED).random((STEPS, N, 8), dtype=np.float32) * 2 - 1).astype(np.float32)


def make_env(fused, device=DEV):
    import isaacgymenvs_amd
    env = isaacgymenvs_amd.make(seed=SEED, task="Ant", num_envs=N, sim_device=device, rl_device=device, headless=True)
    if device != "cpu":
        env.engine.set_option("multi_wave", 16)
        env.engine.set_option("fused_sub", fused)
        env.engine.set_option("fused_post", fused)
        assert int(env.engine.get_option("multi_wave")) == 16 and int(env.engine.get_option("fused_sub")) == fused
        assert int(env.engine.get_option("fused_post")) == fused
    return env


def _put_down(env):
    import torch
    root = env.engine.tensors["root_states"]
    r = root.clone()
    low = torch.as_tensor(LOW, device=r.device, dtype=torch.int64)
    r[low, 2] = LOW_Z
    r[low, 3:7] = torch.tensor([0.0, 0.0, 0.0, 1.0], device=r.device)
    r[low, 7:13] = 0.0
    flipped = torch.as_tensor(FLIPPED, device=r.device, dtype=torch.int64)
    r[flipped, 2] = FLIPPED_Z
    r[flipped, 3:7] = torch.tensor([1.0, 0.0, 0.0, 0.0], device=r.device)
    r[flipped, 9] = FLIPPED_VZ
    rolled = torch.as_tensor(ROLLED, device=r.device, dtype=torch.int64)
    half = np.deg2rad(115.0)
    r[rolled, 2] = FLIPPED_Z
    r[rolled, 3:7] = torch.tensor([float(np.sin(half)), 0.0, 0.0, float(np.cos(half))], device=r.device)
    r[rolled, 9] = FLIPPED_VZ
    root[:] = r


def rollout(env, acts):
    """STEPS control steps; the arrays of ARRAYS after every step, as numpy [STEPS, ...]"""
    import torch
    dev = env.engine.tensors["root_states"].device
    env.step(torch.zeros((N, 8), device=dev))         # (a fresh env resets every env in its first step)
    env.reset_buf[torch.as_tensor(FLAGGED_AT_START, device=dev, dtype=torch.int64)] = 1
    out = {k: [] for k in ARRAYS}
    t = env.engine.tensors
    for step in range(STEPS):
        _put_down(env)
        obs, rew, reset, _ = env.step(torch.as_tensor(acts[step], device=dev))
        now = {"obs": obs["obs"], "rew": rew, "reset": reset, "root": t["root_states"], "dof": t["dof_state"],
               "contact_impulse": t["contact_impulse"], "force_sensor": t["force_sensor"]}
        for k in ARRAYS:
            out[k].append(now[k].detach().cpu().numpy().copy())
    return {k: np.stack(v) for k, v in out.items()}


@pytest.fixture(scope="module")
def runs():
    acts = actions()
    return rollout(make_env(1), acts), rollout(make_env(0), acts)


def test_trunk_contacts_one_launch_equals_separate_launches(runs):
    one, sep = runs
    for k in ARRAYS:
        for step in range(STEPS):
            assert np.array_equal(one[k][step], sep[k][step]), (k, step)


def test_trunk_contacts_equal_the_recorded_arrays(runs):
    one, _ = runs
    g = np.load(GOLDEN)
    assert np.array_equal(g["actions"], actions())
    for k in ARRAYS:
        assert one[k].dtype == g[k].dtype and one[k].shape == g[k].shape, k
        for step in range(STEPS):
            assert np.array_equal(one[k][step], g[k][step]), (k, step)


def test_trunk_contacts_are_exercised(runs):
    """the torso sphere (contact sphere 0) presses on the ground in workgroups 0 and 1 after every step -- in some lanes of workgroup 0 only -- and no
    trunk sphere (0 .. 4) ever does in workgroup 2; envs were reset on the way"""
    one, _ = runs
    ci = one["contact_impulse"]                      # [STEPS, N, 13, 3]: normal + two tangent impulses per sphere
    others = [e for e in range(16) if e not in LOW_WG0]
    for step in range(STEPS):
        print("step", step, "envs with a torso impulse:", np.nonzero(ci[step, :, 0, 0])[0].tolist(), "with a hip-stub impulse:",
              np.nonzero(np.abs(ci[step, :, 1:5]).sum((1, 2)))[0].tolist())
        assert np.isfinite(ci[step]).all()
        assert (ci[step, :16, 0, 0] > 0).any() and (ci[step, 16:32, 0, 0] > 0).any(), step
        assert not ci[step, others, :5].any() and not ci[step, 32:, :5].any(), step
    assert one["reset"].sum() > 0
