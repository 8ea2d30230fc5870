"""GPU test of the Ant's one-launch control step (csrc/mw_kernels.hpp substep_mw_fused_post_kernel) at the batch sizes where its post step can go
wrong: the role waves take their foot-sensor columns from the registers the last sub-step's output phase left them in, and the trunk wave loads
every per-env scalar of the post step (reset flag, episode, progress, potential, running return, randomize counter) in one group at its head."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = 60
SENS = slice(28, 52)        # the 24 force-sensor columns of the Ant's 60 observations (12 root, 8 + 8 dof, 24 sensor, 8 action columns)
TENSORS = ("root_states", "dof_state", "contact_impulse", "limit_impulse", "potentials", "prev_potentials", "progress_buf", "episode_count", "obs_buf",
           "rew_buf", "reset_buf", "up_vec", "heading_vec", "randomize_buf", "timeout_buf", "force_sensor", "dof_force", "episode_return")


def _forced_resets(n):
    """step -> envs whose reset flag is set before that step: a fixed subset with the last env, once every env"""
    some = sorted({0, n // 2, n - 1})
    return {10: some, 25: list(range(n)), 35: [n - 1], 47: some}


# 1: one live lane; 16: exactly one workgroup; 17: a second workgroup with one live lane (its other lanes retire before the early loads);
# 48 with 32 envs per workgroup: the 32-env form, its second workgroup half empty
@pytest.mark.parametrize("n,mw", [(1, 16), (16, 16), (17, 16), (48, 32)])
def test_ant_one_launch_step_matches_the_separate_launches(n, mw):
    """Two Ant engines side by side over 60 steps of seeded random actions: one on the one-launch form (fused_sub = 1, fused_post = 1), the other on one
    launch per sub-step plus loco_post_kernel, which reads every tensor from memory (fused_sub = 0, fused_post = 0).  Resets are forced at fixed
    steps on both.  Observations, rewards, reset flags and every state / output tensor are bit-identical; the ants do touch the ground."""
    import isaacgymenvs_amd
    a = isaacgymenvs_amd.make(seed=4, task="Ant", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True)
    b = isaacgymenvs_amd.make(seed=4, task="Ant", num_envs=n, sim_device=DEV, rl_device=DEV, headless=True)
    for env, fused in ((a, 1), (b, 0)):
        env.engine.set_option("multi_wave", mw)
        env.engine.set_option("fused_sub", fused)
        env.engine.set_option("fused_post", fused)
        assert int(env.engine.get_option("multi_wave")) == mw and int(env.engine.get_option("fused_sub")) == fused
        assert int(env.engine.get_option("fused_post")) == fused
    forced = _forced_resets(n)
    g = torch.Generator(device=DEV).manual_seed(0)
    touched = False
    episodes0 = a.engine.tensors["episode_count"].clone()
    for step in range(STEPS):
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
    assert torch.allclose(a.engine.tensors["episode_stats"], b.engine.tensors["episode_stats"], rtol=1e-4)     # (sums of atomics: the order differs)
    assert touched, "no foot ever touched the ground: the sensor columns were never exercised"
    assert int((a.engine.tensors["episode_count"] - episodes0).min()) >= 1, "an env was never reset"
