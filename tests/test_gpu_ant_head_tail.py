"""GPU tests of the head and the tail of the one-launch control step (csrc/mw_kernels.hpp substep_mw_fused_post_kernel, substep_mw_fused_kernel):
every argument line is fetched at kernel entry and the state, the actions and the warm-start impulses are loaded in one group; every sub-step of a
launch but the last skips the output phase of its P5 (core/engine_mw.hpp substep_role, `outputs`); the job statistics are formed by a leg wave from
the scalars the trunk wave publishes, with DPP row sums and one add of N for the count of env-steps.  None of that changes a value: the one-launch
form stays bit-identical to one launch per sub-step plus the post kernel."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENS = slice(28, 52)        # the 24 force-sensor columns of the Ant's 60 observations
TENSORS = ("root_states", "dof_state", "contact_impulse", "limit_impulse", "potentials", "prev_potentials", "progress_buf", "episode_count", "obs_buf",
           "rew_buf", "reset_buf", "up_vec", "heading_vec", "randomize_buf", "timeout_buf", "force_sensor", "dof_force", "episode_return")


def _forced_resets(n):
    """step -> envs whose reset flag is set before that step: a fixed subset with the last env, once every env"""
    some = sorted({0, n // 2, n - 1})
    return {10: some, 25: list(range(n)), 35: [n - 1], 47: some}


def _ant_pair(n, mw, cfi):
    import isaacgymenvs_amd
    a = isaacgymenvs_amd.make(seed=4, task="Ant", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True)
    b = isaacgymenvs_amd.make(seed=4, task="Ant", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True)
    for env, fused in ((a, 1), (b, 0)):
        env.engine.set_option("multi_wave", mw)
        env.engine.set_option("fused_sub", fused)
        env.engine.set_option("fused_post", fused)
        if cfi != 1:
            env.engine.set_option("control_freq_inv", cfi)
            assert int(env.engine.get_option("control_freq_inv")) == cfi
        assert int(env.engine.get_option("multi_wave")) == mw and int(env.engine.get_option("fused_sub")) == fused
        assert int(env.engine.get_option("fused_post")) == fused
    return a, b


# (n, envs per workgroup, control_freq_inv) -- 1: one live lane; 16: exactly one workgroup; 17: a second workgroup with one live lane; 200: 13 workgroups,
# the last partly empty; 48 with 32 envs per workgroup: the 32-env form (two DPP rows), its second workgroup half empty; control_freq_inv 3 at n = 40:
# six sub-steps per launch, five of them with the outputs skipped
@pytest.mark.parametrize("n,mw,cfi", [(1, 16, 1), (16, 16, 1), (17, 16, 1), (200, 16, 1), (48, 32, 1), (40, 16, 3)])
def test_ant_one_launch_step_head_and_tail(n, mw, cfi):
    """Two Ant engines side by side over 60 steps of seeded random actions with resets forced at fixed steps (the last env included): the one-launch form
    (fused_sub = 1, fused_post = 1) against one launch per sub-step plus loco_post_kernel.  Observations, rewards and reset flags are bit-identical
    every step, the 18 state / output tensors at the end.  Job statistics: the count of env-steps (entry 4) is steps * n exactly on both engines (integers
    below 2^24 are exact in fp32) and the count of finished episodes (entry 2) is the same integer; the three sums of floats (finished returns and lengths,
    rewards) are added in another order: rtol 1e-4."""
    steps = 60
    a, b = _ant_pair(n, mw, cfi)
    forced = _forced_resets(n)
    g = torch.Generator(device=DEV).manual_seed(0)
    touched = False
    episodes0 = a.engine.tensors["episode_count"].clone()
    stats0 = [env.engine.tensors["episode_stats"].clone() for env in (a, b)]
    for step in range(steps):
        if step in forced:
            ids = torch.as_tensor(forced[step], device=DEV, dtype=torch.int64)
            a.reset_buf[ids] = 1
            b.reset_buf[ids] = 1
        act = torch.rand((n, 8), device=DEV, generator=g) * 2 - 1
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        assert torch.equal(oa["obs"], ob["obs"]) and torch.equal(ra, rb) and torch.equal(da, db), step
        touched = touched or bool((oa["obs"][:, SENS] != 0).any())
    for k in TENSORS:
        assert torch.equal(a.engine.tensors[k], b.engine.tensors[k]), k
    sa, sb = (env.engine.tensors["episode_stats"] - s0 for env, s0 in zip((a, b), stats0))
    print("episode_stats one-launch", sa.tolist(), "separate launches", sb.tolist())
    assert float(sa[4]) == float(steps * n) and float(sb[4]) == float(steps * n)
    assert float(sa[2]) == float(sb[2])          # (a forced reset is not a finished episode: only an env the reward terminates counts)
    for k in (0, 1, 3):
        assert torch.allclose(sa[k], sb[k], rtol=1e-4), k
    assert touched, "no foot ever touched the ground: the sensor columns were never exercised"
    assert int((a.engine.tensors["episode_count"] - episodes0).min()) >= 1, "an env was never reset"


def test_anymal_terrain_one_launch_sub_steps_skip_dead_outputs():
    """AnymalTerrain at n = 48 (three workgroups of 16, or two of 32 with the second half empty), fused_sub 1 against 0 over 30 steps: the launch holds
    the decimation sub-steps and the base class's simulate(); only its last sub-step writes impulses, joint forces and net contact forces, the
    refreshed dof-state tensor is written where the decimation loop ends.  Every tensor is bit-identical and the feet do press on the terrain."""
    import isaacgymenvs_amd
    n, steps = 48, 30
    a = isaacgymenvs_amd.make(seed=5, task="AnymalTerrain", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True)
    b = isaacgymenvs_amd.make(seed=5, task="AnymalTerrain", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True)
    assert int(a.engine.get_option("multi_wave")) in (16, 32)
    a.engine.set_option("fused_sub", 1); b.engine.set_option("fused_sub", 0)
    assert int(a.engine.get_option("fused_sub")) == 1 and int(b.engine.get_option("fused_sub")) == 0
    g = torch.Generator(device=DEV).manual_seed(0)
    foot_force = 0.0
    feet = a.feet_indices.to(DEV).long()
    for step in range(steps):
        if step == 12:
            ids = torch.as_tensor([0, n - 1], device=DEV, dtype=torch.int64)
            a.reset_buf[ids] = 1
            b.reset_buf[ids] = 1
        act = torch.rand((n, 12), device=DEV, generator=g) * 2 - 1
        oa, ra, da, _ = a.step(act)
        ob, rb, db, _ = b.step(act)
        assert torch.equal(oa["obs"], ob["obs"]) and torch.equal(ra, rb) and torch.equal(da, db), step
        foot_force = max(foot_force, float(a.engine.tensors["net_contact_force"][:, feet].abs().max()))
    names = [k for k in TENSORS if k in a.engine.tensors] + ["net_contact_force", "dof_state_refreshed", "dof_actuation_force"]
    assert {"root_states", "dof_state", "contact_impulse", "limit_impulse", "progress_buf", "obs_buf", "rew_buf", "reset_buf", "dof_force"} <= set(names)
    for k in names:
        assert torch.equal(a.engine.tensors[k], b.engine.tensors[k]), k
    assert foot_force > 0.0, "no foot ever pressed on the terrain"
