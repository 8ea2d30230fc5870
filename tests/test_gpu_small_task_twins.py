"""The pre / post / reset bodies of Quadcopter, Ingenuity and BallBalance are ONE definition (csrc/tasks/*_step.hpp) that the HIP kernels run
per lane and the CPU backend per loop iteration.  hipcc contracts a * b + c into an FMA unless told otherwise and the CPU library is built
with -ffp-contract=off, so the tensors that only these bodies write -- no physics result feeds them -- must hold the same bits on both
libraries; a MI_NO_CONTRACT that went missing (or appeared) on the way into the shared header shows here.

70 envs: the last wave of every kernel is partly filled.  The arenas start out full of NaN patterns (MI_ARENA_POISON), so a tensor that one
side leaves alone differs from what the other side writes.  Every env is compared."""
import pytest
import torch

from isaacgymenvs_amd import native

N = 70
COMMON = ["actions", "progress_buf", "episode_count", "randomize_buf"]
OWN = {"Quadcopter": ["dof_position_targets", "thrusts", "forces"],
       "Ingenuity": ["thrusts", "forces", "target_root_positions", "marker_states"],
       "BallBalance": ["dof_position_targets"]}


def _engines(task, monkeypatch):
    import isaacgymenvs_amd
    monkeypatch.setenv("MI_ARENA_POISON", "1")
    env = isaacgymenvs_amd.make(seed=3, task=task, num_envs=N, sim_device="cpu", rl_device="cpu", headless=True)
    sim, tp = env.engine._sim, env.engine._tp
    hip, cpu = (native.Engine(task, sim, tp, N, dev, seed=3) for dev in ("cuda:0", "cpu"))
    assert set(hip.tensors) == set(cpu.tensors)
    return hip, cpu


def _step(hip, cpu, g):
    a = torch.rand((N, hip.tensors["actions"].shape[1]), generator=g) * 4 - 2        # beyond clip_actions on both sides: the clamp is exercised
    hip.step(a.to("cuda:0"))
    cpu.step(a)
    torch.cuda.synchronize()


def _differing(task, hip, cpu):
    def bits(t):
        return t.cpu().contiguous().flatten().view(torch.uint8)

    differ = [name for name in COMMON + OWN[task] if not torch.equal(bits(hip.tensors[name]), bits(cpu.tensors[name]))]
    print(task, "compared:", COMMON + OWN[task], "differ:", differ)
    return differ


@pytest.mark.gpu
@pytest.mark.parametrize("task", list(OWN))
def test_first_step_writes_the_same_bits_on_both_libraries(task, monkeypatch):
    """init_state, then exactly one step: reset_buf starts at 1, so every env takes the deferred reset of the pre step."""
    hip, cpu = _engines(task, monkeypatch)
    assert bool((cpu.tensors["reset_buf"] == 1).all()) and bool((hip.tensors["reset_buf"] == 1).all())
    _step(hip, cpu, torch.Generator().manual_seed(5))
    assert bool((cpu.tensors["episode_count"] == 1).all()) and bool((cpu.tensors["progress_buf"] == 1).all())
    assert not _differing(task, hip, cpu)


@pytest.mark.gpu
@pytest.mark.parametrize("task", list(OWN))
def test_action_integration_writes_the_same_bits_on_both_libraries(task, monkeypatch):
    """In the first step the reset overrides what the pre step integrates (targets + dt * scale * a, the thrusts).  A second step with reset_buf
    cleared by hand on both sides -- so that no physics result decides who resets -- runs that arithmetic from the first step's bit-equal
    targets and thrusts on nobody's reset path."""
    hip, cpu = _engines(task, monkeypatch)
    g = torch.Generator().manual_seed(5)
    _step(hip, cpu, g)
    hip.tensors["reset_buf"].zero_()
    cpu.tensors["reset_buf"].zero_()
    _step(hip, cpu, g)
    assert bool((cpu.tensors["episode_count"] == 1).all()) and bool((cpu.tensors["progress_buf"] == 2).all())
    moved = cpu.tensors[OWN[task][0]]
    assert bool((moved != 0).any()) and bool(torch.isfinite(moved).all())
    assert not _differing(task, hip, cpu)
