"""Scenes with more than four static boxes: the WIDE form of the scene sub-step (csrc/core/scene_engine.hpp SceneSim<M, 12>: 64-bit broad-phase mask,
12 statics in the work area, the statics a block of their own), the build define MI_SCENE_STATIC_CAP of a variant (assets/runtime.py), the export
mi_engine_set_scene_statics and the stand-in's route to them (5 to 12 static boxes in prepare_sim).

The robot, the scene builder, the sim settings and the tolerances are those of tests/test_scene_shapes.py (dt 1/60, 2 sub-steps, 8 + 1 iterations,
contact offset 5 mm; 1.5 mm on staying on a face, 0.05 m/s of rest).  The pen: eight wall boxes in a ring (inner apothem 0.2 m) around a slab at z = 1,
the slab the LAST static -- nine statics.  Every scene also asserts that no contact was refused for want of a slot."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_scene_shapes import ARM, G, I4, SLAB_T, TOP, _quat, _refused, _run, _scene  # noqa: F401  (ARM: the robot _scene compiles)

EDGE = 0.05                                 # the cubes' edge
CX, CY = 0.5, 0.0                           # the pen's axis
APO, WALL_T, WALL_H = 0.2, 0.04, 0.12       # inner apothem of the ring, thickness and height of a wall box
WALL_Z = TOP + WALL_H / 2 - 0.02            # the walls stand 2 cm deep in the slab: no edge of a cube's face lies ON an edge of a wall's face (a tie of the outline clipping)
H = 1.0 / 120.0                             # one sub-step


def _dir(k, n=8):
    th = 2.0 * np.pi * k / n
    return th, np.array([np.cos(th), np.sin(th), 0.0])


def _pen():
    """statics of the pen: walls 0..7 (wall k faces the axis from direction 2 pi k / 8, neighbours meet at the outer radius), the slab LAST"""
    hw = (APO + WALL_T) * np.tan(np.pi / 8)
    walls = []
    for k in range(8):
        th, u = _dir(k)
        walls.append(((WALL_T, 2 * hw, WALL_H), (CX + (APO + WALL_T / 2) * u[0], CY + (APO + WALL_T / 2) * u[1], WALL_Z), _quat([0, 0, 1], th)))
    return walls + [((0.6, 0.6, SLAB_T), (CX, CY, 1.0), I4)]


def _commit(gym, sim, root, actor, state):
    """teleport: per-env rows [n, 13] of one actor, committed by index"""
    n, na = root.shape[0], root.shape[1]
    root[:, actor] = torch.as_tensor(state, dtype=torch.float32, device=root.device)
    ids = (torch.arange(n, device=root.device, dtype=torch.int32) * na + actor).contiguous()
    gym.set_actor_root_state_tensor_indexed(sim, root.view(-1, 13), ids, len(ids))


def _launch_states(n, edge_on=False):
    """env k: the cube 1 cm in front of wall k % 8, facing it (edge_on: an upright edge first), at 0.5 m/s towards it"""
    s = np.zeros((n, 13))
    for e in range(n):
        th, u = _dir(e % 8)
        s[e, 0:3] = np.array([CX, CY, TOP + EDGE / 2]) + u * (APO - (EDGE / np.sqrt(2.0) if edge_on else EDGE / 2) - 0.01)
        s[e, 3:7] = _quat([0, 0, 1], th + (np.pi / 4 if edge_on else 0.0))
        s[e, 7:10] = 0.5 * u
    return s


def _inside_pen(x):
    """how far the cube centres [n, 3] are beyond (inner apothem - half edge), worst wall"""
    return max(float(((x - np.array([CX, CY, 0.0])) @ _dir(k)[1]).max()) for k in range(8)) - (APO - EDGE / 2)


# ---------------------------------------------------------------------------------------------------------------- 1. the pen holds
def _pen_holds(device):
    n = 8
    gym, sim, arm, root = _scene(device, _pen(), [("box", (EDGE,) * 3, (CX, CY, TOP + EDGE / 2), I4)], n=n)
    assert sim.scene[9] == ("static", 8) and sim.scene[10] == ("free", 0) and len(sim.scene_statics) == 9
    assert sim.engine.get_option("scene_static_capacity") == 12
    _commit(gym, sim, root, 10, _launch_states(n))
    most = np.zeros(n, int)
    for _ in range(60):
        _run(gym, sim, 1)
        most = np.maximum(most, sim.engine.tensors["scene_contacts"][:, 0].cpu().numpy())
    x = root[:, 10].cpu().numpy()
    print("pen:", np.abs(x[:, 7:10]).max(), _inside_pen(x[:, :3]), x[:, 2] - (TOP + EDGE / 2), most)
    assert _refused(sim) == 0
    assert (most >= 8).all(), most                  # four corners on the slab (static 8) and four on wall k (statics 0..7) at once
    assert np.linalg.norm(x[:, 7:10], axis=1).max() < 0.05
    assert _inside_pen(x[:, :3]) < 1.5e-3
    assert np.abs(x[:, 2] - (TOP + EDGE / 2)).max() < 1.5e-3


def test_pen_of_eight_walls_holds_the_cube_cpu():
    _pen_holds("cpu")


@pytest.mark.gpu
def test_pen_of_eight_walls_holds_the_cube_hip():
    _pen_holds("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 2. parity against the oracle
ARM_AT = (0.017, -0.399, 0.87)              # the straight arm swings its tip (a sphere of radius 0.03 at 0.5 m) against the OUTER face of wall 6
PRESS_ENV, PRESS_Q = 6, np.radians(15.0) + 0.15


def _tip(q):
    """the forearm's end (the centre of its last collision sphere) from the joint angles [n, 2]"""
    a, b = q[:, 0], q[:, 0] + q[:, 1]
    return np.stack([ARM_AT[0] + 0.25 * np.cos(a) + 0.25 * np.cos(b), ARM_AT[1] + 0.25 * np.sin(a) + 0.25 * np.sin(b)], axis=1)


def _oracle(sim, arm, n):
    from oracle.scene import OracleSceneEngine
    es, tp, P = arm.engine_spec, sim.engine._tp, sim.engine._sim
    prm = dict(dt=P.dt, substeps=P.substeps, iters=P.iters, gravity=tuple(P.gravity), contact_offset=P.contact_offset, rest_offset=P.rest_offset,
               max_depen_vel=P.max_depen_vel, erp=P.erp, plane_mu=P.plane_mu, ground_z=P.ground_z, cfm=P.cfm, warm=P.warm)
    sc = tp.scene
    scene = dict(arm_gravity=bool(sc.arm_gravity), arm_mu=float(sc.arm_mu),
                 free=[dict(half=list(sc.free_half[i]), mass=float(sc.free_mass[i]), inertia=list(sc.free_inertia[i]), mu=float(sc.free_mu[i]),
                            pose=list(sc.free_init[i])) for i in range(sc.n_free)],
                 static=[dict(s) for s in sim.scene_statics])
    orc = OracleSceneEngine(es, n, prm, scene, kp=[tp.kp[d] for d in range(es.nd)], kd=[tp.kd[d] for d in range(es.nd)],
                            drive_vmax=[tp.drive_vmax[d] for d in range(es.nd)])
    orc.root[:] = sim.engine.tensors["root_states"].cpu().numpy()
    return orc


def _pen_parity(device):
    """The pen against oracle/scene.py, thresholds of tests/test_scene.py::_parity (poses 1e-3, velocities 5e-2, equal contact counts, joint
    positions 5e-4), 30 steps.  The oracle is unchanged and its warm-start keys were written for at most four statics -- `1 + si * 8 + 4 + s` is
    unique only for s <= 3, `(i * 8 + cr) * 9 + (t + 1)` only for t <= 7 -- so the scene stays where they cannot collide: exactly ONE free body, nine
    statics, the elevated slab last and no ground-plane contact, the arm touching one wall only (wall 6, in one env) and no free body.
    The cubes hit their walls EDGE first (an upright edge: 4 contacts on the slab + 2 on the wall, and they come to rest).  Face first, a cube ends up
    pressed flat against the wall with 8 contacts on its 6 dofs, and the product AND the oracle settle into the same two-step cycle of +-0.02 rad/s
    (below every rest threshold, test 1) whose phase is arbitrary: 0.04 to 0.07 rad/s between two trajectories that are both right -- a limit cycle
    cannot be compared step by step.
    Known answer behind it: the driven joint stops at the wall -- the tip sphere's centre stands one radius off the wall's face, to 1.5 mm."""
    n = 8
    gym, sim, arm, root = _scene(device, _pen(), [("box", (EDGE,) * 3, (CX, CY, TOP + EDGE / 2), I4)], n=n, arm_at=ARM_AT, drive=(20.0, 2.0))
    es = arm.engine_spec
    tip = [s for s in range(len(es.sph_body)) if es.sph_body[s] == 2 and abs(es.sph_pos[s][0] - 0.25) < 1e-6]
    assert tip and abs(es.sph_rad[tip[0]] - 0.03) < 1e-6, (es.sph_pos, es.sph_rad)           # the sphere _tip() follows
    cube = _launch_states(n, edge_on=True)
    _commit(gym, sim, root, 10, cube)
    tg = np.zeros((n, 2)); tg[PRESS_ENV, 0] = PRESS_Q
    gym.set_dof_position_target_tensor(sim, torch.tensor(tg, dtype=torch.float32, device=sim.device).view(-1))
    orc = _oracle(sim, arm, n)
    orc.targets[:] = tg
    orc.box[:, 0] = cube
    dof = gym.acquire_dof_state_tensor(sim).view(n, 2, 2)
    arm_touch = 0
    for step in range(30):
        gym.simulate(sim)
        orc.step(np.zeros((n, 2)))
        gym.refresh_actor_root_state_tensor(sim); gym.refresh_dof_state_tensor(sim)
        got = root[:, 10].cpu().numpy()
        d = np.abs(got - orc.box[:, 0])
        d[..., 3:7] = np.minimum(d[..., 3:7], np.abs(got[..., 3:7] + orc.box[:, 0, 3:7]))
        nc = sim.engine.tensors["scene_contacts"].cpu().numpy()
        print("parity:", step, d[..., :7].max(), d[..., 7:].max(), nc[:, 0], orc.ncontacts, np.abs(dof[..., 0].cpu().numpy() - orc.q).max())
        assert d[..., :7].max() < 1e-3 and d[..., 7:].max() < 5e-2, (step, d[..., :7].max(), d[..., 7:].max())
        assert (nc[:, 0] == orc.ncontacts).all(), (step, nc[:, 0], orc.ncontacts)
        np.testing.assert_allclose(dof[..., 0].cpu().numpy(), orc.q, atol=5e-4)
        arm_touch += int(nc[PRESS_ENV, 0] > nc[(PRESS_ENV + 1) % n, 0])
    assert arm_touch > 10 and _refused(sim) == 0
    for _ in range(60):
        gym.simulate(sim)
    gym.refresh_dof_state_tensor(sim)
    q = dof[..., 0].cpu().numpy()
    ty = _tip(q)[:, 1]
    face = CY - (APO + WALL_T)                       # wall 6 faces -y: its outer face
    print("press:", q[PRESS_ENV], _tip(q)[PRESS_ENV], face - 0.03, dof[PRESS_ENV, :, 1])
    assert abs(ty[PRESS_ENV] - (face - 0.03)) < 1.5e-3 and float(dof[PRESS_ENV, :, 1].abs().max()) < 0.05
    assert q[PRESS_ENV, 0] < PRESS_Q - 0.05          # stopped short of its target
    assert abs(_tip(q)[PRESS_ENV, 0] - CX) < 0.06    # on the face, away from the neighbours' corners


def test_pen_follows_the_oracle_and_the_wall_stops_the_arm_cpu():
    _pen_parity("cpu")


@pytest.mark.gpu
def test_pen_follows_the_oracle_and_the_wall_stops_the_arm_hip():
    _pen_parity("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 3. full house
def _full_house_scene():
    """12 statics: the slab (0), seven pillars standing clear of everything (1..7), four walls of a square yard (8..11: +x, +y, -x, -y).  Free bodies:
    three cubes lying flat, yawed 45 degrees, one upright edge against wall 8 / 9 / 10 near a corner of the yard (4 corners on the slab + 2 on the
    wall each), and a sphere (free body 3) on the slab against wall 11: 3 * 6 + 2 = 20 contacts for the 24 slots."""
    a, t = 0.22, 0.04
    statics = [((0.6, 0.6, SLAB_T), (CX, CY, 1.0), I4)]
    statics += [((0.03, 0.03, 0.06), (CX - 0.09 + 0.03 * k, CY, TOP + 0.03), I4) for k in range(7)]
    for k in range(4):
        th, u = _dir(k, 4)
        statics.append(((t, 2 * (a + t), WALL_H), (CX + (a + t / 2) * u[0], CY + (a + t / 2) * u[1], WALL_Z), _quat([0, 0, 1], th)))
    r = EDGE / np.sqrt(2.0)                          # centre to upright edge
    frees = []
    for k in range(3):
        th, u = _dir(k, 4)
        v = np.array([-u[1], u[0], 0.0])
        p = np.array([CX, CY, TOP + EDGE / 2 + 0.004]) + u * (a - r) + v * (a - 0.07)
        frees.append(("box", (EDGE,) * 3, tuple(p), _quat([0, 0, 1], th + np.pi / 4)))
    th, u = _dir(3, 4)
    frees.append(("sphere", (0.03,), tuple(np.array([CX, CY, TOP + 0.03 + 0.004]) + u * (a - 0.03) + np.array([0.1, 0.0, 0.0])), I4))
    return statics, frees


def _fids(nsph, nstat=12, nfree=4):
    """feature ids of the wide form (csrc/core/scene_engine.hpp): corner (i, cr) against target t (-1 ground, statics, then free bodies) and round body
    i, point e, against target tt (0 ground, 1 + static, 1 + 12 + free).  A LAYOUT PIN: these formulas restate FID_SC / FID_EE / FID_FC / FID_RD of
    scene_engine.hpp for NSTAT = 12 and change with them (the net contact force tensor has no rows for free bodies; scene_warm is where their
    impulses can be read)"""
    ntgt = nfree + nstat
    corner0 = 1 + nsph * ntgt
    fid_sc = corner0 + nfree * 8 * (ntgt + 1)
    fid_rd = fid_sc + nstat * 8 * nfree + nfree * ntgt * 9 + nfree * ntgt * 8
    return ntgt, corner0, fid_rd


def _t2z(n):
    """z component of the second tangent of a contact whose normal is n (csrc/core/engine.hpp contact_frame: t1 = x made orthogonal to n -- y when n
    is +-x --, t2 = n x t1)"""
    n = np.asarray(n, float)
    a = np.array([1.0, 0.0, 0.0]) - n[0] * n
    t1 = a / np.linalg.norm(a) if a @ a > 1e-12 else np.array([0.0, 1.0, 0.0])
    return float(np.cross(n, t1)[2])


def _full_house(device):
    n = 8
    statics, frees = _full_house_scene()
    gym, sim, arm, root = _scene(device, statics, frees, n=n)
    assert len(sim.scene_statics) == 12 and sim.scene[12] == ("static", 11) and sim.scene[16] == ("free", 3)
    _run(gym, sim, 60)
    T = sim.engine.tensors
    x = root[:, 13:17].cpu().numpy()
    nc = T["scene_contacts"].cpu().numpy()
    warm = T["scene_warm"].cpu().numpy()                            # [n, 48, 4]: feature (int bits), normal and tangent impulses
    fid = warm[..., 0].copy().view(np.int32)
    print("full house:", nc[0], np.abs(x[..., 7:]).max(), x[0, :, 2])
    assert _refused(sim) == 0 and (nc[:, 0] == 20).all(), nc
    assert np.abs(x[..., 7:10]).max() < 0.05 and np.abs(x[:, :3, 10:13]).max() < 0.05         # at rest: 0.05 m/s, 0.05 rad/s for the cubes
    assert np.abs(x[:, 3, 10:13]).max() * 0.03 < 0.05                                         # (the sphere may still roll: its surface speed r w)
    assert np.abs(x[:, :3, 2] - (TOP + EDGE / 2)).max() < 1.5e-3 and np.abs(x[:, 3, 2] - (TOP + 0.03)).max() < 1.5e-3
    ntgt, corner0, fid_rd = _fids(len(arm.engine_spec.sph_body))
    sc = sim.engine._tp.scene
    for e in range(n):
        used = fid[e] > 0
        seen = set()
        for i in range(4):
            # the weight of body i is on its contact rows (last sub-step's impulses / h): the normal rows against the slab (static 0, normal +z) and
            # the friction of its wall contact (normal -u of wall 8 + i, horizontal: of its frame only the second tangent has a z component).  (The
            # engine's net contact force tensor has rows for the ACTOR's bodies only, and the oracle's keys do not hold for this scene: the rows
            # are read from tensor scene_warm by their feature ids.)
            if i < 3:
                ids = [corner0 + (i * 8 + cr) * (ntgt + 1) + (0 + 1) for cr in range(8)]
            else:
                ids = [fid_rd + (i * (ntgt + 1) + 1 + 0) * 4 + 0]
            rows = np.isin(fid[e], ids) & used
            lam = warm[e, rows, 1]
            mg = float(sc.free_mass[i]) * G
            assert rows.sum() == (4 if i < 3 else 1) and (lam > 0).all(), (e, i, lam)
            # and the body touches ITS wall, static 8 + i: two corners of a cube's upright edge / the sphere
            if i < 3:
                wall = [corner0 + (i * 8 + cr) * (ntgt + 1) + (8 + i + 1) for cr in range(8)]
            else:
                wall = [fid_rd + (i * (ntgt + 1) + 1 + 11) * 4 + 0]
            wrows = np.isin(fid[e], wall) & used
            assert wrows.sum() == (2 if i < 3 else 1), (e, i, fid[e][used])
            fz = (float(lam.sum()) + float(warm[e, wrows, 3].sum()) * _t2z(-_dir(i, 4)[1])) / H
            if e == 0:
                print("weight of body", i, fz, mg, "of it wall friction", float(warm[e, wrows, 3].sum()) * _t2z(-_dir(i, 4)[1]) / H)
            assert abs(fz - mg) < 0.03 * mg + 1e-3, (e, i, fz, mg)
            seen.update(ids + wall)
        assert set(fid[e][used].tolist()) <= seen


def test_full_house_twelve_statics_four_bodies_rest_on_their_contacts_cpu():
    _full_house("cpu")


@pytest.mark.gpu
def test_full_house_twelve_statics_four_bodies_rest_on_their_contacts_hip():
    _full_house("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 4. capacity equivalence
def _three_static_run(device, wide, monkeypatch, n=16):
    """a slab, a low wall and a tilted block; a cube, a sphere and a capsule dropped and pushed at them from per-env states; 30 steps"""
    statics = [((0.6, 0.6, SLAB_T), (CX, CY, 1.0), I4), ((0.04, 0.6, 0.12), (CX + 0.2, CY, TOP + 0.04), I4),
               ((0.1, 0.1, 0.04), (CX - 0.1, CY + 0.15, TOP + 0.02), _quat([1, 0, 0], 0.2))]
    frees = [("box", (EDGE,) * 3, (CX, CY, TOP + 0.1), I4), ("sphere", (0.03,), (CX, CY - 0.15, TOP + 0.1), I4),
             ("capsule", (0.03, 0.2), (CX - 0.1, CY - 0.05, TOP + 0.2), I4)]
    if wide:
        monkeypatch.setenv("MI_SHIM_STATIC_CAPACITY", "12")
    else:
        monkeypatch.delenv("MI_SHIM_STATIC_CAPACITY", raising=False)
    gym, sim, arm, root = _scene(device, statics, frees, n=n)
    assert sim.engine.get_option("scene_static_capacity") == (12 if wide else 4) and len(sim.scene_statics) == 3
    rng = np.random.default_rng(11)
    for a_, (_, _, p0, _) in zip((4, 5, 6), frees):
        s = np.zeros((n, 13))
        s[:, 0:3] = np.array(p0) + rng.uniform(-0.02, 0.02, (n, 3)) + [0.0, 0.0, 0.02]
        ax = rng.normal(size=(n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        ang = rng.uniform(0.0, 0.3, n)
        s[:, 3:6], s[:, 6] = ax * np.sin(ang / 2)[:, None], np.cos(ang / 2)
        s[:, 7:10] = rng.uniform(-0.3, 0.3, (n, 3)) * [1.0, 1.0, 0.3] + [0.4, 0.0, 0.0]
        _commit(gym, sim, root, a_, s)
    _run(gym, sim, 30)
    assert _refused(sim) == 0
    return root[:, 4:7].cpu().numpy().copy(), sim.engine.tensors["scene_contacts"].cpu().numpy().copy()


def _per_env(a, b):
    d = np.abs(a - b)
    d[..., 3:7] = np.minimum(d[..., 3:7], np.abs(a[..., 3:7] + b[..., 3:7]))
    return d[..., :7].reshape(len(a), -1).max(axis=1)


def _capacity_equivalence(device, monkeypatch):
    (xa, ca), (xb, cb) = _three_static_run(device, False, monkeypatch), _three_static_run(device, True, monkeypatch)
    per_env = _per_env(xa, xb)
    print("capacity 4 against 12:", device, np.quantile(per_env, 0.99), per_env.max(), ca[:, 0], cb[:, 0])
    assert np.isfinite(xb).all() and ca[:, 0].max() >= 4
    assert np.quantile(per_env, 0.99) < 2e-4 and per_env.max() < 5e-3, (np.quantile(per_env, 0.99), per_env.max())


def test_three_statics_run_the_same_at_capacity_4_and_12_cpu(monkeypatch):
    _capacity_equivalence("cpu", monkeypatch)


@pytest.mark.gpu
def test_three_statics_run_the_same_at_capacity_4_and_12_hip(monkeypatch):
    _capacity_equivalence("cuda:0", monkeypatch)


# ---------------------------------------------------------------------------------------------------------------- 5. ragged batch
@pytest.mark.gpu
def test_pen_hip_matches_the_cpu_backend_on_a_ragged_batch():
    """13 envs of the pen (a multiple of neither 4 nor 8 envs per workgroup): random cube poses and velocities, HIP against the CPU backend"""
    n = 13
    rng = np.random.default_rng(7)
    s = np.zeros((n, 13))
    s[:, 0:2] = np.array([CX, CY]) + rng.uniform(-0.1, 0.1, (n, 2))
    s[:, 2] = TOP + EDGE / 2 + rng.uniform(0.0, 0.03, n)
    ax = rng.normal(size=(n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = rng.uniform(0.0, 0.4, n)
    s[:, 3:6], s[:, 6] = ax * np.sin(ang / 2)[:, None], np.cos(ang / 2)
    th = rng.uniform(0.0, 2 * np.pi, n)
    s[:, 7], s[:, 8] = 0.8 * np.cos(th), 0.8 * np.sin(th)
    out = {}
    for device in ("cpu", "cuda:0"):
        gym, sim, arm, root = _scene(device, _pen(), [("box", (EDGE,) * 3, (CX, CY, TOP + EDGE / 2), I4)], n=n)
        _commit(gym, sim, root, 10, s)
        _run(gym, sim, 30)
        assert _refused(sim) == 0
        out[device] = (root[:, 10:11].cpu().numpy().copy(), sim.engine.tensors["scene_contacts"].cpu().numpy().copy())
    per_env = _per_env(out["cuda:0"][0], out["cpu"][0])
    print("ragged pen:", np.quantile(per_env, 0.99), per_env.max(), out["cuda:0"][1][:, 0])
    assert np.isfinite(out["cuda:0"][0]).all() and out["cuda:0"][1][:, 0].max() >= 6           # somebody is at a wall
    assert np.quantile(per_env, 0.99) < 2e-4 and per_env.max() < 5e-3, (np.quantile(per_env, 0.99), per_env.max())


# ---------------------------------------------------------------------------------------------------------------- 6. the export
def _set_statics(eng, n, pos, quat, half, mu):
    arr = lambda v: None if v is None else (C.c_float * len(v))(*v)          # noqa: E731
    rc = eng.L.mi_engine_set_scene_statics(eng.h, n, arr(pos), arr(quat), arr(half), arr(mu))
    return rc, (eng.L.mi_last_error() or b"").decode()


def test_set_scene_statics_refusals_and_capacity_cpu(monkeypatch):
    """mi_engine_set_scene_statics on the CPU library (host arena, nothing is simulated): every refusal of include/mi_engine.h with its message;
    scene_static_capacity 4 on a variant built as ever, 12 on a wide one; 12 boxes accepted, 13 refused"""
    from isaacgymenvs_amd import native
    slab = [((0.6, 0.6, SLAB_T), (CX, CY, 1.0), I4)]
    cube = [("box", (EDGE,) * 3, (CX, CY, TOP + EDGE / 2), I4)]
    monkeypatch.delenv("MI_SHIM_STATIC_CAPACITY", raising=False)
    _, sim4, _, _ = _scene("cpu", slab, cube)
    monkeypatch.setenv("MI_SHIM_STATIC_CAPACITY", "12")
    _, sim12, _, _ = _scene("cpu", slab, cube)
    e4, e12 = sim4.engine, sim12.engine
    assert e4.get_option("scene_static_capacity") == 4 and e12.get_option("scene_static_capacity") == 12
    assert e4.L._name != e12.L._name                                   # two cached libraries of one robot
    with pytest.raises(RuntimeError, match="read-only"):
        e12.set_option("scene_static_capacity", 4)
    box = lambda n: ([0.0, 0.0, 1.0] * n, [0.0, 0.0, 0.0, 1.0] * n, [0.1, 0.1, 0.1] * n, [0.5] * n)          # noqa: E731
    for eng, cap in ((e4, 4), (e12, 12)):
        assert _set_statics(eng, cap, *box(cap))[0] == 0
        rc, msg = _set_statics(eng, cap + 1, *box(cap + 1))
        assert rc != 0 and f"holds {cap}" in msg, msg
        rc, msg = _set_statics(eng, -1, *box(1))
        assert rc != 0 and "n < 0" in msg, msg
        for drop in range(4):
            args = list(box(2)); args[drop] = None
            rc, msg = _set_statics(eng, 2, *args)
            assert rc != 0 and "null array" in msg, msg
        assert _set_statics(eng, 0, None, None, None, None)[0] == 0          # no static boxes: no arrays needed
        p, q, h, m = box(2)
        for bad in (0.0, -0.1):
            rc, msg = _set_statics(eng, 2, p, q, h[:4] + [bad] + h[5:], m)
            assert rc != 0 and "static box 1" in msg and "half size" in msg, msg
        for bad in (1.002, 0.998, 0.0):
            rc, msg = _set_statics(eng, 2, p, q[:3] + [bad] + q[4:], h, m)
            assert rc != 0 and "static box 0" in msg and "quaternion" in msg, msg
        assert _set_statics(eng, 2, p, q[:3] + [1.0005] + q[4:], h, m)[0] == 0
    # the set replaces the whole static set; the first four are what MiScene shows
    assert e12.set_scene_statics([dict(pos=[k, 0, 1], quat=I4, half=[0.1, 0.2, 0.3], mu=0.25) for k in range(9)]) is None
    # not a fixed-base Articulation scene: the stock library's robot has a floating base
    tp = native.MiArticulationParams()
    tp.init_root[2], tp.init_root[6] = 0.9, 1.0
    amp = native.Engine("Articulation", e4._sim, tp, 2, "cpu")
    rc, msg = _set_statics(amp, 1, *box(1))
    assert rc != 0 and "fixed-base Articulation" in msg, msg
    assert amp.get_option("scene_static_capacity") == 4
    with pytest.raises(ValueError):
        from isaacgymenvs_amd.assets import runtime
        runtime.variant_library("articulation", None, "cpu", static_capacity=8)


def test_more_than_twelve_statics_are_refused_cpu():
    statics = [((0.03, 0.03, 0.06), (CX - 0.2 + 0.03 * k, CY, TOP + 0.03), I4) for k in range(13)]
    with pytest.raises(NotImplementedError, match="at most 12 static boxes"):
        _scene("cpu", statics, [("box", (EDGE,) * 3, (CX, CY + 0.2, TOP + EDGE / 2), I4)])


# ---------------------------------------------------------------------------------------------------------------- 7. ring decomposition
RING_IN, RING_OUT, RING_H, RING_N = 0.2, 0.25, 0.1, 64


def _write_ring(tmp):
    """a procedural annulus (a 64-gon, inner radius 0.2, outer 0.25, height 0.1, its axis the mesh frame's z) as an ASCII STL + a one-body URDF;
    -> its vertices [4 * 64, 3]"""
    import os
    a = 2 * np.pi * np.arange(RING_N) / RING_N
    P = {(s, z): np.stack([r * np.cos(a), r * np.sin(a), np.full(RING_N, z)], axis=1) for s, r in (("i", RING_IN), ("o", RING_OUT)) for z in (0.0, RING_H)}
    tris = []
    for i in range(RING_N):
        j = (i + 1) % RING_N
        for q in ((P["o", 0.0][i], P["o", 0.0][j], P["o", RING_H][j], P["o", RING_H][i]), (P["i", 0.0][j], P["i", 0.0][i], P["i", RING_H][i], P["i", RING_H][j]),
                  (P["i", RING_H][i], P["o", RING_H][i], P["o", RING_H][j], P["i", RING_H][j]), (P["i", 0.0][j], P["o", 0.0][j], P["o", 0.0][i], P["i", 0.0][i])):
            tris += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    with open(os.path.join(tmp, "ring.stl"), "w") as f:
        f.write("solid ring\n")
        for t in tris:
            f.write("facet normal 0 0 0\nouter loop\n" + "".join("vertex %.9g %.9g %.9g\n" % tuple(v) for v in t) + "endloop\nendfacet\n")
        f.write("endsolid ring\n")
    with open(os.path.join(tmp, "ring.urdf"), "w") as f:
        f.write('<robot name="ring"><link name="ring"><collision><origin xyz="0 0 0" rpy="0 0 0"/><geometry><mesh filename="ring.stl"/></geometry>'
                '</collision></link></robot>\n')
    return np.concatenate(list(P.values()))


def _box_distance(b, p):
    """distance of the points p [n, 3] to the box b (dict pos / quat (a yaw) / half)"""
    yaw = 2.0 * np.arctan2(b["quat"][2], b["quat"][3])
    c, s = np.cos(yaw), np.sin(yaw)
    d = p - np.asarray(b["pos"])
    loc = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1], d[:, 2]], axis=1)
    out = np.maximum(np.abs(loc) - np.asarray(b["half"]), 0.0)
    return np.sqrt((out * out).sum(1))


def _load_ring(tmp, monkeypatch, k):
    import warnings

    import isaacgymenvs_amd.shims as shims
    shims.install(force=True)
    from isaacgym import gymapi
    V = _write_ring(str(tmp))
    if k is None:
        monkeypatch.delenv("MI_SHIM_RING_WALLS", raising=False)
    else:
        monkeypatch.setenv("MI_SHIM_RING_WALLS", str(k))
    gym = gymapi.acquire_gym()
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, gymapi.SimParams())
    o = gymapi.AssetOptions(); o.fix_base_link = True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        a = gym.load_asset(sim, str(tmp), "ring.urdf", o)
    return a, V, [str(x.message) for x in w]


def test_ring_mesh_becomes_eight_wall_boxes_cpu(tmp_path, monkeypatch):
    """MI_SHIM_RING_WALLS=8 on a procedural annulus: 8 boxes, none reaches inside the inner radius, every OUTER vertex lies in a box (1 mm), the warning
    names 8 and the worst gap; unset or 0: today's warning and no boxes.  INNER vertices: the issue asks for 1 mm as well, which cannot hold beside
    `no box inside radius 0.2` -- a flat face tangent at the sector's middle stands r_in (1 - cos(pi / 8)) = 15.2 mm off the round inner surface at
    the sector's edge -- so they are held to that analytic gap, and the gap the warning names is checked against it."""
    a, V, msgs = _load_ring(tmp_path, monkeypatch, 8)
    boxes = a.ring_boxes
    assert len(boxes) == 8 and gym_one_body(a)
    r = np.hypot(V[:, 0], V[:, 1])
    for b in boxes:
        yaw = 2.0 * np.arctan2(b["quat"][2], b["quat"][3])
        u = np.array([np.cos(yaw), np.sin(yaw)])
        # tangent box: its point nearest to the axis is the middle of its inner face
        assert abs(np.asarray(b["pos"][:2]) @ u - np.hypot(*b["pos"][:2])) < 1e-9 and np.hypot(*b["pos"][:2]) - b["half"][0] >= RING_IN - 1e-9, b
        assert abs(np.hypot(*b["pos"][:2]) + b["half"][0] - RING_OUT) < 1e-9 and abs(b["half"][2] - RING_H / 2) < 1e-9 and abs(b["pos"][2] - RING_H / 2) < 1e-9
        assert abs(b["half"][1] - RING_OUT * np.tan(np.pi / 8)) < 1e-9                       # neighbours meet at the outer radius
    dist = np.min([_box_distance(b, V) for b in boxes], axis=0)
    gap = RING_IN * (1.0 - np.cos(np.pi / 8))
    print("ring: worst outer", dist[r > 0.225].max(), "worst inner", dist[r < 0.225].max(), "analytic", gap, msgs)
    assert dist[r > 0.225].max() < 1e-3
    assert dist[r < 0.225].max() < gap + 1e-6 and dist[r < 0.225].max() > gap - 1e-3
    assert len(msgs) == 1 and "8 static wall boxes" in msgs[0] and f"{gap * 1e3:.1f} mm" in msgs[0] and "WITHOUT a collision shape" not in msgs[0], msgs
    for k in (None, 0):
        a, _, msgs = _load_ring(tmp_path, monkeypatch, k)
        assert a.ring_boxes is None and a.hollow and len(msgs) == 1 and "WITHOUT a collision shape" in msgs[0], msgs
    monkeypatch.setenv("MI_SHIM_RING_WALLS", "12")
    with pytest.raises(ValueError, match="4 to 11"):
        _load_ring(tmp_path, monkeypatch, 12)


def gym_one_body(a):
    return len(a.body_names) == 1 and a.nshapes == 1


def _ring_scene(device, tmp, monkeypatch, k):
    """the test arm far away, a slab, the ring standing on it (a one-body URDF, fix_base_link) and a cube inside; two envs"""
    import os

    import isaacgymenvs_amd.shims as shims
    from isaacgymenvs_amd import native
    if device == "cpu":
        native.build_cpu()
    shims.install(force=True)
    from isaacgym import gymapi
    _write_ring(str(tmp))
    with open(os.path.join(str(tmp), "scene_arm2.xml"), "w") as f:
        f.write(ARM)
    if k is None:
        monkeypatch.delenv("MI_SHIM_RING_WALLS", raising=False)
    else:
        monkeypatch.setenv("MI_SHIM_RING_WALLS", str(k))
    gym = gymapi.acquire_gym()
    sp = gymapi.SimParams()
    sp.up_axis, sp.gravity, sp.dt, sp.substeps, sp.use_gpu_pipeline = gymapi.UP_AXIS_Z, gymapi.Vec3(0, 0, -G), 1 / 60.0, 2, device != "cpu"
    sp.physx.num_position_iterations, sp.physx.num_velocity_iterations = 8, 1
    sp.physx.contact_offset, sp.physx.rest_offset = 0.005, 0.0
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, sp)
    gym.add_ground(sim, gymapi.PlaneParams())
    opts = gymapi.AssetOptions()
    opts.fix_base_link, opts.disable_gravity, opts.default_dof_drive_mode = True, True, gymapi.DOF_MODE_EFFORT
    arm = gym.load_asset(sim, str(tmp), "scene_arm2.xml", opts)
    fixed = gymapi.AssetOptions(); fixed.fix_base_link = True
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ring = gym.load_asset(sim, str(tmp), "ring.urdf", fixed)
    slab = gym.create_box(sim, 0.6, 0.6, SLAB_T, fixed)
    cube = gym.create_box(sim, EDGE, EDGE, EDGE, gymapi.AssetOptions())
    for a_ in (slab, cube):
        pr = gym.get_asset_rigid_shape_properties(a_)
        pr[0].friction = 0.5
        gym.set_asset_rigid_shape_properties(a_, pr)
    T = lambda p_: gymapi.Transform(gymapi.Vec3(*[float(x) for x in p_]), gymapi.Quat(0.0, 0.0, 0.0, 1.0))  # noqa: E731
    n = 2
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 2)
        gym.create_actor(env, arm, T((-2.5, 0.0, 1.0)), "arm", i, 0, 0)
        gym.create_actor(env, slab, T((CX, CY, 1.0)), "slab", i, 1, 0)
        gym.create_actor(env, ring, T((CX, CY, TOP)), "ring", i, 1, 0)
        gym.create_actor(env, cube, T((CX, CY, TOP + EDGE / 2)), "cube", i, 2, 0)
    gym.prepare_sim(sim)
    root = gym.acquire_actor_root_state_tensor(sim).view(n, 4, 13)
    return gym, sim, root


def _ring_holds(device, tmp_path, monkeypatch):
    """a cube pushed at 0.5 m/s towards a sector's middle (env 0) and towards a sector's edge (env 1) stays inside the ring's outer radius"""
    gym, sim, root = _ring_scene(device, tmp_path, monkeypatch, 8)
    assert sim.scene == {1: ("static", 0), 2: ("walls", 1, 8), 3: ("free", 0)} and len(sim.scene_statics) == 9 and sim.nactors == 4
    assert sim.engine.get_option("scene_static_capacity") == 12
    s = np.zeros((2, 13))
    for e, (th, r0) in enumerate(((np.pi / 8, RING_IN - EDGE / 2 - 0.01), (np.pi / 4, RING_IN / np.cos(np.pi / 8) - EDGE / 2 - 0.02))):
        # sector 0 spans 0 .. 45 degrees: towards its middle (the flat inner face, 1 cm ahead), towards its edge (the groove where two faces meet)
        u = np.array([np.cos(th), np.sin(th), 0.0])
        s[e, 0:3] = np.array([CX, CY, TOP + EDGE / 2]) + u * r0
        s[e, 3:7] = _quat([0, 0, 1], th)
        s[e, 7:10] = 0.5 * u
    _commit(gym, sim, root, 3, s)
    most = np.zeros(2, int)
    for _ in range(60):
        _run(gym, sim, 1)
        most = np.maximum(most, sim.engine.tensors["scene_contacts"][:, 0].cpu().numpy())
    x = root[:, 3].cpu().numpy()
    rad = np.hypot(x[:, 0] - CX, x[:, 1] - CY)
    print("ring holds:", rad, np.abs(x[:, 7:10]).max(), most)
    assert _refused(sim) == 0 and (most > 4).all()                  # more than the four corners on the slab: a wall was touched
    assert (rad + EDGE * np.sqrt(0.5) < RING_OUT).all() and np.abs(x[:, 2] - (TOP + EDGE / 2)).max() < 1.5e-3 and np.abs(x[:, 7:10]).max() < 0.05


def test_ring_walls_hold_a_cube_at_a_sector_middle_and_edge_cpu(tmp_path, monkeypatch):
    _ring_holds("cpu", tmp_path, monkeypatch)


@pytest.mark.gpu
def test_ring_walls_hold_a_cube_at_a_sector_middle_and_edge_hip(tmp_path, monkeypatch):
    _ring_holds("cuda:0", tmp_path, monkeypatch)


def test_ring_without_the_switch_has_no_collision_shape_cpu(tmp_path, monkeypatch):
    gym, sim, root = _ring_scene("cpu", tmp_path, monkeypatch, None)
    assert sim.scene == {1: ("static", 0), 3: ("free", 0)} and len(sim.scene_statics) == 1
    assert sim.engine.get_option("scene_static_capacity") == 4


# ---------------------------------------------------------------------------------------------------------------- 8. the reference's trifinger.py
from test_scene import REF, TRIFINGER, franka_task  # noqa: E402, F401  (the fixture that imports the reference's task files over the stand-ins)


@pytest.mark.skipif(not __import__("os").path.isfile(TRIFINGER), reason="the reference's trifinger assets are not reachable")
def test_reference_trifinger_with_ring_walls_keeps_the_cube_in_the_arena_cpu(franka_task, monkeypatch):
    """the unmodified trifinger.py with MI_SHIM_RING_WALLS=8: its boundary becomes eight static boxes beside the table plate (9 statics, the wide
    library), 80 random steps leave finite buffers, and a cube teleported to the rim with 1 m/s outwards is still inside the boundary's outer radius
    one second later.  CPU only: the reference's files are where the CPU tests run."""
    import os

    from isaacgymenvs_amd import native
    from isaacgymenvs_amd.utils.config import compose, omegaconf_to_dict
    native.build_cpu()
    monkeypatch.setenv("MI_SHIM_RING_WALLS", "8")
    mod0, vt = franka_task
    mod = mod0.load("trifinger")
    assert os.path.samefile(mod.__file__, os.path.join(REF, "isaacgymenvs", "tasks", "trifinger.py"))
    vt.EXISTING_SIM = None
    n = 16
    cfg = omegaconf_to_dict(compose("config", overrides=["task=Trifinger"], cfg_dir=os.path.join(REF, "isaacgymenvs", "cfg"))["task"])
    cfg["env"]["numEnvs"], cfg["sim"]["use_gpu_pipeline"] = n, False
    torch.manual_seed(3)
    with pytest.warns(UserWarning, match="8 static wall boxes"):
        env = mod.Trifinger(cfg, rl_device="cpu", sim_device="cpu", graphics_device_id=-1, headless=True, virtual_screen_capture=False, force_render=False)
    sim = env.sim
    assert sim.scene == {1: ("static", 0), 2: ("walls", 1, 8), 3: ("free", 0)} and sim.nactors == 5 and len(sim.scene_statics) == 9
    assert sim.engine.get_option("scene_static_capacity") == 12
    walls = sim.scene_statics[1:]
    r_out = max(np.hypot(*w["pos"][:2]) + w["half"][0] for w in walls)
    r_in = min(np.hypot(*w["pos"][:2]) - w["half"][0] for w in walls)
    print("trifinger boundary: inner", r_in, "outer", r_out, "z", walls[0]["pos"][2], walls[0]["half"])
    g = torch.Generator().manual_seed(0)
    for step in range(80):
        obs, rew, reset, _ = env.step((torch.rand((n, 9), generator=g) * 2 - 1))
        assert torch.isfinite(obs["obs"]).all() and torch.isfinite(rew).all(), step
    for t in sim.engine.tensors.values():
        if t.dtype == torch.float32:
            assert torch.isfinite(t).all()
    # the cube at the rim, 1 m/s outwards, env k in direction 2 pi k / n
    sc = sim.engine.tensors["scene_state"]
    half = 0.0325
    for e in range(n):
        th = 2 * np.pi * e / n
        u = np.array([np.cos(th), np.sin(th)])
        s = torch.zeros(13)
        s[0:2] = torch.tensor(u * (r_in - 2.5 * half), dtype=torch.float32)
        s[2], s[6] = half, 1.0
        s[7:9] = torch.tensor(u * 1.0, dtype=torch.float32)
        sc[e, 0] = s
    for _ in range(int(round(1.0 / (cfg["sim"]["dt"])))):
        env.gym.simulate(sim)
    cube = sc[:, 0].cpu().numpy()
    print("cube radius after 1 s:", np.hypot(cube[:, 0], cube[:, 1]))
    assert np.isfinite(cube).all() and (np.hypot(cube[:, 0], cube[:, 1]) < r_out).all(), np.hypot(cube[:, 0], cube[:, 1])
