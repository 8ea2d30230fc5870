"""Scenes whose free bodies are not all boxes: spheres and capsules beside a fixed-base arm (csrc/core/scene_engine.hpp, MiScene.free_shape).

The file carries its own robot -- a two-hinge fixed-base arm written as an MJCF string, compiled at run time -- so that it runs where the
reference's assets are not.  oracle/scene.py knows boxes only; the evidence here is first principles (a round body has closed-form ROLLING
answers that test the normal row, both tangent rows, the friction disc and the inertia at once) and the two product backends against each
other.  Sim settings and tolerances are those of tests/test_scene.py: dt 1/60, 2 sub-steps, 8 + 1 iterations, contact offset 5 mm; 5 % on a
velocity, 8 % + 1 mm on a distance, 1.5 mm on staying on a face, 1.5 frames on a landing time, 0.05 m/s of rebound.  Every scene also asserts
that no contact was refused for want of a slot."""
import os
import tempfile

import numpy as np
import pytest
import torch

G = 9.81
ARM = """<mujoco model="scene_arm2">
  <compiler angle="degree" inertiafromgeom="true"/>
  <default><joint armature="0.02" damping="0.5" limited="true"/><geom density="900" friction="1.0 0.5 0.5"/></default>
  <worldbody>
    <body name="base" pos="0 0 0">
      <geom name="base_geom" type="capsule" fromto="0 0 0 0 0 0.2" size="0.05"/>
      <body name="upper" pos="0 0 0.2">
        <joint name="shoulder" type="hinge" axis="0 0 1" range="-170 170"/>
        <geom name="upper_geom" type="capsule" fromto="0 0 0 0.25 0 0" size="0.03"/>
        <body name="fore" pos="0.25 0 0">
          <joint name="elbow" type="hinge" axis="0 0 1" range="-150 150"/>
          <geom name="fore_geom" type="capsule" fromto="0 0 0 0.25 0 0" size="0.03"/>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator><motor joint="shoulder" gear="40"/><motor joint="elbow" gear="40"/></actuator>
</mujoco>
"""
I4 = [0.0, 0.0, 0.0, 1.0]
R_S = 0.03                      # the spheres' radius
CAP_R, CAP_L = 0.03, 0.2        # the capsules: radius, length of the cylinder part (axis: local x)
SLAB_T = 0.04                   # thickness of the slabs and ramps; their centres stand at z = 1
TOP = 1.0 + SLAB_T / 2
FAR = (-2.5, 0.0, 1.0)          # where the arm stands when a scene is about the bodies alone


def _quat(axis, rad):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    return list(a * np.sin(rad / 2)) + [float(np.cos(rad / 2))]


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
            aw * bw - ax * bx - ay * by - az * bz]


def _rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _scene(device, statics, frees, n=2, mu=0.5, gravity=-G, arm_at=FAR, drive=None):
    """the test arm (actor 0) in a scene: statics = [(size3, position3, quaternion xyzw)] static boxes, frees = [(kind, dims, position3,
    quaternion xyzw)] with kind "box" (dims: 3 sizes), "sphere" (radius,) or "capsule" (radius, length); shape friction mu on every asset.
    drive = (stiffness, damping): the arm's dofs are position drives.  -> gym, sim, arm asset, root tensor view [n, actors, 13]"""
    import isaacgymenvs_amd.shims as shims
    from isaacgymenvs_amd import native
    if device == "cpu":
        native.build_cpu()
    shims.install(force=True)
    from isaacgym import gymapi
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "scene_arm2.xml"), "w") as f:
        f.write(ARM)
    gym = gymapi.acquire_gym()
    sp = gymapi.SimParams()
    sp.up_axis, sp.gravity, sp.dt, sp.substeps, sp.use_gpu_pipeline = gymapi.UP_AXIS_Z, gymapi.Vec3(0, 0, gravity), 1 / 60.0, 2, device != "cpu"
    sp.physx.num_position_iterations, sp.physx.num_velocity_iterations = 8, 1
    sp.physx.contact_offset, sp.physx.rest_offset = 0.005, 0.0
    sim = gym.create_sim(0, -1, gymapi.SIM_PHYSX, sp)
    gym.add_ground(sim, gymapi.PlaneParams())
    opts = gymapi.AssetOptions()
    opts.fix_base_link, opts.disable_gravity, opts.default_dof_drive_mode = True, True, gymapi.DOF_MODE_EFFORT
    arm = gym.load_asset(sim, tmp, "scene_arm2.xml", opts)
    assert arm.generic and gym.get_asset_dof_count(arm) == 2
    fixed = gymapi.AssetOptions(); fixed.fix_base_link = True

    def asset(kind, dims, o):
        dims = [float(x) for x in dims]
        a_ = {"box": gym.create_box, "sphere": gym.create_sphere, "capsule": gym.create_capsule}[kind](sim, *dims, o)
        pr = gym.get_asset_rigid_shape_properties(a_)
        pr[0].friction = mu
        gym.set_asset_rigid_shape_properties(a_, pr)
        return a_
    sa = [asset("box", sz, fixed) for sz, _, _ in statics]
    fa = [asset(kind, dims, gymapi.AssetOptions()) for kind, dims, _, _ in frees]
    T = lambda p_, q_: gymapi.Transform(gymapi.Vec3(*[float(x) for x in p_]), gymapi.Quat(*[float(x) for x in q_]))  # noqa: E731
    dp = gym.get_asset_dof_properties(arm)
    if drive is not None:
        dp["driveMode"][:], dp["stiffness"][:], dp["damping"][:] = gymapi.DOF_MODE_POS, drive[0], drive[1]
    for i in range(n):
        env = gym.create_env(sim, gymapi.Vec3(), gymapi.Vec3(), 2)
        h = gym.create_actor(env, arm, T(arm_at, I4), "arm", i, 0, 0)
        gym.set_actor_dof_properties(env, h, dp)
        for k, (a_, (_, p_, q_)) in enumerate(zip(sa, statics)):
            gym.create_actor(env, a_, T(p_, q_), f"static{k}", i, 1, 0)
        for k, (a_, (_, _, p_, q_)) in enumerate(zip(fa, frees)):
            gym.create_actor(env, a_, T(p_, q_), f"free{k}", i, 2, 0)
    gym.prepare_sim(sim)
    root = gym.acquire_actor_root_state_tensor(sim).view(n, 1 + len(statics) + len(frees), 13)
    return gym, sim, arm, root


def _refused(sim):
    return int(sim.engine.tensors["scene_contacts"][:, 1].sum())


def _run(gym, sim, frames):
    for _ in range(frames):
        gym.simulate(sim)
    gym.refresh_actor_root_state_tensor(sim)


def _set_velocity(gym, sim, root, actor, lin):
    """teleport: the actor's rows of the root tensor with a linear velocity, committed by index (franka_cube_stack.py:505-511)"""
    n, na = root.shape[0], root.shape[1]
    root[:, actor, 7:10] = torch.tensor(lin, dtype=torch.float32, device=root.device)
    ids = (torch.arange(n, device=root.device, dtype=torch.int32) * na + actor).contiguous()
    gym.set_actor_root_state_tensor_indexed(sim, root.view(-1, 13), ids, len(ids))


def _slab(length=0.6):
    return ((length, 0.6, SLAB_T), (0.5, 0.0, 1.0), I4)


def _ramp(angle_deg, length=1.2):
    """a slab pitched about +y (its +x end goes DOWN): -> static box, angle, face normal, down-slope direction, its quaternion"""
    th = np.radians(angle_deg)
    q = _quat([0, 1, 0], th)
    return ((length, 0.6, SLAB_T), (0.5, 0.0, 1.0), q), th, np.array([np.sin(th), 0.0, np.cos(th)]), np.array([np.cos(th), 0.0, -np.sin(th)]), q


def _on_ramp(nrm, down, radius, along=-0.3):
    return np.array([0.5, 0.0, 1.0]) + nrm * (SLAB_T / 2 + radius) + down * along


# ---------------------------------------------------------------------------------------------------------------- 1. drop and rest
def _drop_and_rest(device):
    """a sphere dropped from h = 12 cm above a static slab lands after sqrt(2 h / g), does not bounce, rests with its centre r above the face"""
    h = 0.12
    gym, sim, arm, root = _scene(device, [_slab()], [("sphere", (R_S,), (0.5, 0.0, TOP + R_S + h), I4)])
    t_hit, vmax_up = None, 0.0
    for k in range(90):
        _run(gym, sim, 1)
        z, vz = float(root[0, 2, 2]), float(root[0, 2, 9])
        if t_hit is None and z < TOP + R_S + 2e-3:
            t_hit = (k + 1) / 60.0
        if t_hit is not None:
            vmax_up = max(vmax_up, vz)
    x = root[:, 2].cpu().numpy()
    print("drop:", t_hit, np.sqrt(2 * h / G), vmax_up, x[:, 2] - (TOP + R_S))
    assert _refused(sim) == 0
    assert t_hit is not None and abs(t_hit - np.sqrt(2 * h / G)) < 1.5 / 60.0 and vmax_up < 0.05, (t_hit, np.sqrt(2 * h / G), vmax_up)
    assert np.abs(x[:, 2] - (TOP + R_S)).max() < 1.5e-3 and np.abs(x[:, 7:10]).max() < 0.01, x[0]


def test_sphere_dropped_on_a_slab_lands_on_time_and_rests_cpu():
    _drop_and_rest("cpu")


@pytest.mark.gpu
def test_sphere_dropped_on_a_slab_lands_on_time_and_rests_hip():
    _drop_and_rest("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 2., 3. ramps
def _sphere_on_ramp(device, angle_deg, mu, frames=24):
    ramp, th, nrm, down, q = _ramp(angle_deg)
    p0 = _on_ramp(nrm, down, R_S)
    gym, sim, arm, root = _scene(device, [ramp], [("sphere", (R_S,), p0, I4)], mu=mu)
    assert sim.engine._tp.scene.free_mu[0] == np.float32(mu) and sim.engine._tp.scene.static_mu[0] == np.float32(mu)
    _run(gym, sim, frames)
    x = root[:, 2].cpu().numpy()
    assert _refused(sim) == 0
    v = x[:, 7:10] @ down
    rim = np.linalg.norm(np.cross(x[:, 10:13], -R_S * nrm), axis=1)          # speed of the contact point relative to the centre: |w x r|
    return th, frames / 60.0, v, rim, np.linalg.norm(x[:, 10:13], axis=1)


def _rolling_without_slipping(device):
    """ramp 20 degrees, mu = 0.5 (>= 2/7 tan th = 0.104): v = 5/7 g sin th t, and the rim speed |w x r| equals the centre's speed"""
    th, t, v, rim, _ = _sphere_on_ramp(device, 20.0, 0.5)
    want = 5.0 / 7.0 * G * np.sin(th) * t
    print("rolling:", v, rim, want)
    assert np.abs(v - want).max() < 0.05 * want and np.abs(rim - v).max() < 0.05 * want, (v, rim, want)


def test_sphere_rolls_without_slipping_down_a_ramp_cpu():
    _rolling_without_slipping("cpu")


@pytest.mark.gpu
def test_sphere_rolls_without_slipping_down_a_ramp_hip():
    _rolling_without_slipping("cuda:0")


def _slipping(device):
    """ramp 40 degrees, mu = 0.1 (< 2/7 tan th = 0.240): a = g (sin th - mu cos th), angular acceleration 5/2 mu g cos th / r"""
    th, t, v, _, w = _sphere_on_ramp(device, 40.0, 0.1)
    want_v, want_w = G * (np.sin(th) - 0.1 * np.cos(th)) * t, 2.5 * 0.1 * G * np.cos(th) / R_S * t
    print("slipping:", v, want_v, w, want_w)
    assert np.abs(v - want_v).max() < 0.05 * want_v and np.abs(w - want_w).max() < 0.05 * want_w, (v, want_v, w, want_w)


def test_sphere_slips_down_a_steep_ramp_cpu():
    _slipping("cpu")


@pytest.mark.gpu
def test_sphere_slips_down_a_steep_ramp_hip():
    _slipping("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 4. slide to roll
def _slide_to_roll(device):
    """on a level slab a sphere launched at v0 without spin ends up rolling at 5/7 v0 whatever mu is, and keeps that speed"""
    v0 = 1.0
    for mu in (0.3, 0.6):
        slab = ((1.6, 0.6, SLAB_T), (0.5, 0.0, 1.0), I4)
        gym, sim, arm, root = _scene(device, [slab], [("sphere", (R_S,), (-0.1, 0.0, TOP + R_S), I4)], mu=mu)
        _set_velocity(gym, sim, root, 2, [v0, 0.0, 0.0])
        _run(gym, sim, 30)
        x1 = root[:, 2].cpu().numpy().copy()
        _run(gym, sim, 30)
        x2 = root[:, 2].cpu().numpy()
        assert _refused(sim) == 0
        want = 5.0 / 7.0 * v0
        print("slide to roll, mu", mu, x1[:, 7], x1[:, 11] * R_S, x2[:, 7], want)
        assert np.abs(x1[:, 7] - want).max() < 0.05 * want and np.abs(x1[:, 11] * R_S - x1[:, 7]).max() < 0.05 * want, (mu, x1[0, 7:])
        assert np.abs(x2[:, 7] - want).max() < 0.05 * want, (mu, x2[0, 7:])          # no rolling resistance: half a second later
        assert np.abs(x2[:, 2] - (TOP + R_S)).max() < 1.5e-3


def test_sliding_sphere_ends_rolling_at_five_sevenths_cpu():
    _slide_to_roll("cpu")


@pytest.mark.gpu
def test_sliding_sphere_ends_rolling_at_five_sevenths_hip():
    _slide_to_roll("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 5. impacts
def _impacts(device):
    """gravity 0, free space: a sphere at v0 hits an equal sphere at rest head-on -- both go on at v0 / 2 (the contact rows do not bounce); a sphere
    hits a capsule's middle broadside -- both at m_s v0 / (m_s + m_c).  One row gives the two bodies + lambda and - lambda: the total momentum
    differs from m v0 by fp32 rounding only"""
    v0 = 1.0
    for other, dims, gap in (("sphere", (R_S,), 2 * R_S), ("capsule", (CAP_R, CAP_L), R_S + CAP_R)):
        q = I4 if other == "sphere" else _quat([0, 0, 1], np.pi / 2)          # the capsule's axis along y: hit broadside at its middle
        gym, sim, arm, root = _scene(device, [], [("sphere", (R_S,), (0.0, 0.0, 1.5), I4), (other, dims, (gap + 0.05, 0.0, 1.5), q)], gravity=0.0)
        m = [gym.get_actor_rigid_body_properties(sim.envs[0], k)[0].mass for k in (1, 2)]
        _set_velocity(gym, sim, root, 1, [v0, 0.0, 0.0])
        touched = 0
        for _ in range(30):
            _run(gym, sim, 1)
            touched = max(touched, int(sim.engine.tensors["scene_contacts"][:, 0].max()))
        x = root.cpu().numpy()
        va, vb = x[:, 1, 7], x[:, 2, 7]
        want = m[0] * v0 / (m[0] + m[1])
        print("impact", other, va, vb, want, (m[0] * va + m[1] * vb) / (m[0] * v0) - 1)
        assert touched >= 1 and _refused(sim) == 0
        if other == "sphere":
            assert abs(m[0] - m[1]) < 1e-9 and abs(want - v0 / 2) < 1e-12
        assert np.abs(va - want).max() < 0.05 * want and np.abs(vb - want).max() < 0.05 * want, (va, vb, want)
        assert np.abs((m[0] * va + m[1] * vb) / (m[0] * v0) - 1.0).max() < 1e-4
        assert np.abs(x[:, 1:, 8:13]).max() < 1e-3          # central: no sideways velocity, no spin


def test_inelastic_head_on_impacts_conserve_momentum_cpu():
    _impacts("cpu")


@pytest.mark.gpu
def test_inelastic_head_on_impacts_conserve_momentum_hip():
    _impacts("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 6. capsule
def _axis_tilt(x):
    """angle between the capsule's axis (local x) and the horizontal"""
    return np.abs(np.arcsin(np.clip(np.array([_rot(q)[2, 0] for q in x[:, 3:7]]), -1, 1)))


def _capsule(device):
    """(a) lying on the slab a capsule rests at height r, axis level; (b) 40 degree ramp, mu = 0.5, axis ALONG the slope: slides with
    g (sin th - mu cos th) like a cube; (c) 20 degree ramp, axis ACROSS the slope: rolls with a = g sin th / (1 + I_axis / (m r^2)); (d) balanced
    across a thin static box under its middle it stays: the interior contact of its core segment"""
    cap = (CAP_R, CAP_L)
    gym, sim, arm, root = _scene(device, [_slab()], [("capsule", cap, (0.5, 0.0, TOP + CAP_R + 1e-3), I4)])          # (a)
    _run(gym, sim, 60)
    x = root[:, 2].cpu().numpy()
    print("capsule rest:", x[:, 2] - (TOP + CAP_R), _axis_tilt(x), sim.engine.tensors["scene_contacts"][:, 0].tolist())
    assert _refused(sim) == 0 and int(sim.engine.tensors["scene_contacts"][:, 0].min()) == 2             # its two end points
    assert np.abs(x[:, 2] - (TOP + CAP_R)).max() < 1.5e-3 and _axis_tilt(x).max() < 0.01 and np.abs(x[:, 7:]).max() < 0.05
    ramp, th, nrm, down, q = _ramp(40.0)                                                                              # (b)
    p0 = _on_ramp(nrm, down, CAP_R)
    gym, sim, arm, root = _scene(device, [ramp], [("capsule", cap, p0, q)], mu=0.5)
    _run(gym, sim, 24)
    x = root[:, 2].cpu().numpy()
    t, a = 24 / 60.0, G * (np.sin(th) - 0.5 * np.cos(th))
    s, v = (x[:, 0:3] - p0) @ down, x[:, 7:10] @ down
    print("capsule slides:", v, a * t, s, 0.5 * a * t * t)
    assert _refused(sim) == 0
    assert np.abs(v - a * t).max() < 0.05 * a * t and np.abs(s - 0.5 * a * t * t).max() < 0.08 * 0.5 * a * t * t + 1e-3, (s, v, a * t)
    assert np.abs((x[:, 0:3] - p0) @ nrm).max() < 1.5e-3
    ramp, th, nrm, down, q = _ramp(20.0)                                                                              # (c)
    p0 = _on_ramp(nrm, down, CAP_R)
    gym, sim, arm, root = _scene(device, [ramp], [("capsule", cap, p0, _qmul(q, _quat([0, 0, 1], np.pi / 2)))], mu=0.5)
    pr = gym.get_actor_rigid_body_properties(sim.envs[0], 2)[0]
    _run(gym, sim, 24)
    x = root[:, 2].cpu().numpy()
    a = G * np.sin(th) / (1.0 + pr.inertia.x.x / (pr.mass * CAP_R ** 2))
    v = x[:, 7:10] @ down
    print("capsule rolls:", v, a * t, np.abs(x[:, 11]) * CAP_R)
    assert _refused(sim) == 0 and np.abs(v - a * t).max() < 0.05 * a * t, (v, a * t)
    knife = ((0.01, 0.3, 0.2), (0.5, 0.0, 0.9), I4)                                                                   # (d): its top face at z = 1
    gym, sim, arm, root = _scene(device, [knife], [("capsule", cap, (0.5, 0.0, 1.0 + CAP_R + 1e-3), I4)])
    _run(gym, sim, 60)
    x = root[:, 2].cpu().numpy()
    print("capsule on a knife edge:", x[:, 0:3], _axis_tilt(x), sim.engine.tensors["scene_contacts"][:, 0].tolist())
    assert _refused(sim) == 0 and int(sim.engine.tensors["scene_contacts"][:, 0].min()) >= 1
    assert np.abs(x[:, 0:3] - [0.5, 0.0, 1.0 + CAP_R]).max() < 1.5e-3 and _axis_tilt(x).max() < 0.01, (x[0, :3], _axis_tilt(x))


def test_capsule_rests_slides_rolls_and_balances_cpu():
    _capsule("cpu")


@pytest.mark.gpu
def test_capsule_rests_slides_rolls_and_balances_hip():
    _capsule("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 7. stack and mix
def _stack_and_mix(device):
    """(a) a sphere placed on a free cube on the slab stays there, the cube does not sink; (b) a free cube dropped face down onto a resting sphere's
    top is stopped by it: its lowest point stays above 2 r - 1.5 mm while it is over the sphere.  (Dropped from 1 cm: it then travels 3.7 mm per
    sub-step, less than the 5 mm contact offset inside which a contact is seen before it closes.)"""
    c = 0.07
    gym, sim, arm, root = _scene(device, [_slab()], [("box", (c, c, c), (0.5, 0.0, TOP + c / 2), I4), ("sphere", (R_S,), (0.5, 0.0, TOP + c + R_S), I4)])
    _run(gym, sim, 60)
    x = root.cpu().numpy()
    print("sphere on cube:", x[:, 2, 2] - (TOP + c / 2), x[:, 3, 0:3] - [0.5, 0.0, TOP + c + R_S])
    assert _refused(sim) == 0
    assert np.abs(x[:, 2, 2] - (TOP + c / 2)).max() < 1.5e-3 and np.abs(x[:, 3, 0:3] - [0.5, 0.0, TOP + c + R_S]).max() < 1.5e-3
    gym, sim, arm, root = _scene(device, [_slab()], [("sphere", (R_S,), (0.5, 0.0, TOP + R_S), I4), ("box", (c, c, c), (0.5, 0.0, TOP + 2 * R_S + c / 2 + 0.01), I4)])
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * c / 2
    lowest, over = 1e9, 0
    for _ in range(60):
        _run(gym, sim, 1)
        x = root.cpu().numpy()
        for e in range(x.shape[0]):
            if np.abs(x[e, 3, 0:2] - x[e, 2, 0:2]).max() < c / 2:
                over += 1
                lowest = min(lowest, float((x[e, 3, 2] + (_rot(x[e, 3, 3:7]) @ corners.T)[2]).min()) - TOP)
    print("cube on sphere: lowest point", lowest, "frames over the sphere", over)
    assert _refused(sim) == 0 and over >= 20 and lowest > 2 * R_S - 1.5e-3, (lowest, over)


def test_sphere_on_a_cube_and_cube_on_a_sphere_cpu():
    _stack_and_mix("cpu")


@pytest.mark.gpu
def test_sphere_on_a_cube_and_cube_on_a_sphere_hip():
    _stack_and_mix("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 8. the arm pushes a ball
def _arm_pushes_a_ball(device):
    """the arm, stretched out and swept about its shoulder at 1 rad/s by its position drives, pushes a ball lying on the slab with the end of
    its last link; it stops, the ball rolls on.  The ball ends displaced along the push, rolling; no arm sphere ever overlaps it by more than the
    contact offset; the last link's row of the net contact force tensor is non-zero while they touch"""
    n, om, r_ball = 2, 1.0, R_S
    slab = ((0.6, 2.4, SLAB_T), (0.5, 0.0, 1.0), I4)
    ball0 = np.array([0.5, 0.0, TOP + r_ball])
    gym, sim, arm, root = _scene(device, [slab], [("sphere", (r_ball,), ball0, I4)], n=n, arm_at=(0.0, 0.0, TOP + 0.04 - 0.2), drive=(400.0, 40.0))
    es = arm.engine_spec
    sph_b, sph_p, sph_r = np.asarray(es.sph_body), np.asarray(es.sph_pos, float), np.asarray(es.sph_rad, float)
    a0 = -0.5
    ds = torch.zeros((n, 2, 2), device=sim.device); ds[:, 0, 0] = a0
    gym.set_dof_state_tensor(sim, ds.view(-1, 2))
    rb = gym.acquire_rigid_body_state_tensor(sim).view(n, -1, 13)
    netf = gym.acquire_net_contact_force_tensor(sim).view(n, -1, 3)
    fore = gym.find_actor_rigid_body_handle(sim.envs[0], 0, "fore")
    min_gap, touch_force, touching = 1e9, [], 0
    for k in range(110):
        ang = min(a0 + om * (k + 1) / 60.0, 0.1)                      # the sweep stops at 0.1 rad: the ball goes on alone
        tg = torch.zeros((n, 2), device=sim.device); tg[:, 0] = ang
        gym.set_dof_position_target_tensor(sim, tg.view(-1))
        _run(gym, sim, 1)
        gym.refresh_rigid_body_state_tensor(sim); gym.refresh_net_contact_force_tensor(sim)
        body, ball = rb.cpu().numpy(), root[:, 2].cpu().numpy()
        gaps = []
        for e in range(n):
            for s in range(len(sph_b)):
                b = int(sph_b[s])
                if b == 0:
                    continue
                cs = body[e, b, 0:3] + _rot(body[e, b, 3:7]) @ sph_p[s]
                gaps.append(np.linalg.norm(cs - ball[e, 0:3]) - sph_r[s] - r_ball)
        gap = min(gaps)
        min_gap = min(min_gap, gap)
        if gap < 1e-3 and ang < 0.1:               # touching while the sweep goes on (once the arm stops the ball leaves it: no force)
            touching += 1
            touch_force.append(float(np.linalg.norm(netf[:, fore].cpu().numpy(), axis=1).min()))
    ball = root[:, 2].cpu().numpy()
    v = np.linalg.norm(ball[:, 7:9], axis=1)
    rim = np.linalg.norm(np.cross(ball[:, 10:13], [0.0, 0.0, -r_ball]), axis=1)
    print("arm pushes ball: displaced", ball[:, 0:3] - ball0, "v", v, "rim", rim, "min gap", min_gap, "touching frames", touching,
          "forces", touch_force[:3], min(touch_force) if touch_force else None, "last gap", gap)
    assert _refused(sim) == 0
    assert (ball[:, 1] - ball0[1]).min() > 0.05 and np.abs(ball[:, 2] - ball0[2]).max() < 1.5e-3           # pushed along +y, still on the slab
    assert gap > 0.02 and v.min() > 0.05 and np.abs(rim - v).max() < 0.05 * v.max(), (gap, v, rim)          # contact lost, rolling
    assert min_gap > -0.005, min_gap
    assert touching >= 5 and min(touch_force) > 0.0, (touching, touch_force)


def test_arm_pushes_a_ball_which_rolls_on_cpu():
    _arm_pushes_a_ball("cpu")


@pytest.mark.gpu
def test_arm_pushes_a_ball_which_rolls_on_hip():
    _arm_pushes_a_ball("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- 9. ABI / stand-in
def test_free_shape_masses_and_inertias_of_a_mixed_scene_cpu():
    """MiScene.free_shape, free_half, masses and inertias of one box, one sphere, one capsule as include/mi_engine.h specifies them"""
    c, r, (cr, cl) = 0.05, R_S, (CAP_R, CAP_L)
    gym, sim, arm, root = _scene("cpu", [_slab()], [("box", (c, c, c), (0.4, 0.0, TOP + c / 2), I4), ("sphere", (r,), (0.5, 0.0, TOP + r), I4),
                                                    ("capsule", (cr, cl), (0.6, 0.0, TOP + cr), _quat([0, 0, 1], np.pi / 2))])
    sc = sim.engine._tp.scene
    assert sc.n_free == 3 and sc.n_static == 1 and sc.free_shape == (0 | 1 << 4 | 2 << 8)
    assert np.allclose(list(sc.free_half[0]), [c / 2] * 3) and np.allclose(list(sc.free_half[1]), [r] * 3) and np.allclose(list(sc.free_half[2]), [cl / 2, cr, cr])
    rho = 1000.0
    m_s = rho * 4 / 3 * np.pi * r ** 3
    m_cyl, m_caps = rho * np.pi * cr ** 2 * cl, rho * 4 / 3 * np.pi * cr ** 3
    across = m_cyl * (cl ** 2 / 12 + cr ** 2 / 4) + m_caps * (0.4 * cr ** 2 + cl ** 2 / 4 + 0.375 * cl * cr)
    want = [(rho * c ** 3, [rho * c ** 3 * c * c / 6] * 3), (m_s, [0.4 * m_s * r * r] * 3),
            (m_cyl + m_caps, [0.5 * m_cyl * cr ** 2 + 0.4 * m_caps * cr ** 2, across, across])]
    for j, (m, ine) in enumerate(want):
        assert abs(sc.free_mass[j] - m) < 1e-6 * m and np.allclose(list(sc.free_inertia[j]), ine, rtol=1e-6)
        pr = gym.get_actor_rigid_body_properties(sim.envs[0], 2 + j)[0]
        assert abs(pr.mass - m) < 1e-9 * m and np.allclose([pr.inertia.x.x, pr.inertia.y.y, pr.inertia.z.z], ine, rtol=1e-9)
        assert gym.get_actor_rigid_shape_properties(sim.envs[0], 2 + j)[0].friction == 0.5
    # their rows of the root state tensor are those of free boxes: the start poses, teleported by index
    assert np.allclose(root[0, 4, 0:7].numpy(), [0.6, 0.0, TOP + cr] + _quat([0, 0, 1], np.pi / 2), atol=1e-6)
    root[:, 3, 0:3] = torch.tensor([0.45, 0.1, TOP + r + 0.05])
    ids = (torch.arange(2, dtype=torch.int32) * 5 + 3)
    gym.set_actor_root_state_tensor_indexed(sim, root.view(-1, 13), ids, 2)
    assert np.allclose(sim.engine.tensors["scene_state"][:, 1, 0:3].numpy(), [0.45, 0.1, TOP + r + 0.05], atol=1e-6)
    rb = gym.acquire_rigid_body_state_tensor(sim).view(2, -1, 13)
    gym.refresh_rigid_body_state_tensor(sim)
    assert rb.shape[1] == 3 + 1 + 3 and np.allclose(rb[0, 5, 0:3].numpy(), [0.45, 0.1, TOP + r + 0.05], atol=1e-6)
    _run(gym, sim, 30)
    assert _refused(sim) == 0 and abs(float(root[0, 3, 2]) - (TOP + r)) < 1.5e-3


def test_box_only_scene_passes_free_shape_zero_cpu():
    gym, sim, arm, root = _scene("cpu", [_slab()], [("box", (0.05, 0.05, 0.05), (0.5, 0.0, TOP + 0.025), I4)])
    assert sim.engine._tp.scene.free_shape == 0 and sim.engine._tp.scene.n_free == 1
    _run(gym, sim, 10)
    assert _refused(sim) == 0 and abs(float(root[0, 2, 2]) - (TOP + 0.025)) < 1.5e-3


def test_unknown_shape_code_is_refused_by_mi_engine_create_cpu():
    from isaacgymenvs_amd import native
    gym, sim, arm, root = _scene("cpu", [_slab()], [("sphere", (R_S,), (0.5, 0.0, TOP + R_S), I4)])
    eng = sim.engine
    import copy
    tp = copy.deepcopy(eng._tp)
    tp.scene.free_shape = 7
    with pytest.raises(RuntimeError, match="free_shape"):
        native.Engine("Articulation", eng._sim, tp, 2, "cpu", lib_path=eng.L._name)
    tp.scene.free_shape = 2 | 5 << 4            # the code of a body beyond n_free is not looked at
    native.Engine("Articulation", eng._sim, tp, 2, "cpu", lib_path=eng.L._name)


def test_static_sphere_is_not_implemented_cpu():
    import isaacgymenvs_amd.shims as shims
    shims.install(force=True)
    from isaacgym import gymapi
    gym = gymapi.acquire_gym()
    with pytest.raises(NotImplementedError, match="static bodies of a scene are boxes"):
        class _Fixed(tuple):
            pass
        # (_scene gives free bodies default options: build the one static sphere by hand)
        orig = gym.create_sphere
        try:
            def fixed_sphere(sim, radius, options=None):
                o = gymapi.AssetOptions(); o.fix_base_link = True
                return orig(sim, radius, o)
            gym.create_sphere = fixed_sphere
            _scene("cpu", [_slab()], [("sphere", (R_S,), (0.5, 0.0, TOP + R_S), I4)])
        finally:
            del gym.create_sphere


# ---------------------------------------------------------------------------------------------------------------- 10. HIP against the CPU backend
def _ragged_states(n, seed=11):
    """per env a cube, a sphere and a capsule at random poses on / just above the slab and each other, the arm at random poses and targets"""
    rng = np.random.default_rng(seed)
    c = 0.05
    st = np.zeros((3, n, 13)); st[:, :, 6] = 1.0
    base = np.stack([rng.uniform(0.35, 0.65, n), rng.uniform(-0.3, 0.3, n)], axis=1)
    for k, rad in enumerate((c / 2, R_S, CAP_R)):
        st[k, :, 0:2] = base + rng.uniform(-0.09, 0.09, (n, 2))                  # close together: they land on and beside each other
        st[k, :, 2] = TOP + rad + rng.uniform(0.0, 0.006, n) + 0.06 * (rng.random(n) < 0.25)          # a quarter start above the others
        ax = rng.normal(size=(n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
        ang = rng.uniform(0.0, 0.25, n)
        st[k, :, 3:6], st[k, :, 6] = ax * np.sin(ang / 2)[:, None], np.cos(ang / 2)
        st[k, :, 7:10] = rng.uniform(-0.2, 0.2, (n, 3))
    q = rng.uniform(-0.8, 0.8, (n, 2))
    return st, q, q + rng.uniform(-0.4, 0.4, (n, 2))


def _ragged(device, n):
    c = 0.05
    slab = ((0.6, 1.2, SLAB_T), (0.5, 0.0, 1.0), I4)
    gym, sim, arm, root = _scene(device, [slab], [("box", (c, c, c), (0.4, 0.0, 1.2), I4), ("sphere", (R_S,), (0.5, 0.0, 1.2), I4),
                                                  ("capsule", (CAP_R, CAP_L), (0.6, 0.0, 1.2), I4)], n=n, arm_at=(0.0, 0.0, TOP + 0.04 - 0.2), drive=(400.0, 40.0))
    st, q, tg = _ragged_states(n)
    ds = torch.zeros((n, 2, 2), device=sim.device); ds[..., 0] = torch.tensor(q, dtype=torch.float32, device=sim.device)
    gym.set_dof_state_tensor(sim, ds.view(-1, 2))
    gym.set_dof_position_target_tensor(sim, torch.tensor(tg, dtype=torch.float32, device=sim.device).view(-1))
    for k in range(3):
        root[:, 2 + k] = torch.tensor(st[k], dtype=torch.float32, device=sim.device)
    ids = (torch.arange(n, device=sim.device, dtype=torch.int32).view(n, 1) * 5 + torch.tensor([2, 3, 4], device=sim.device, dtype=torch.int32)).flatten()
    gym.set_actor_root_state_tensor_indexed(sim, root.view(-1, 13), ids, len(ids))
    for _ in range(6):
        gym.simulate(sim)
    gym.refresh_actor_root_state_tensor(sim); gym.refresh_dof_state_tensor(sim)
    return root[:, 2:5].cpu().numpy().copy(), sim.engine.tensors["dof_state"].cpu().numpy().copy(), sim.engine.tensors["scene_contacts"].cpu().numpy().copy()


def test_ragged_batch_scenes_hold_round_contacts_and_refuse_none_cpu():
    """the seeded scenes of the HIP-against-CPU comparison below, on the CPU backend alone: no contact refused, and most envs hold contacts of
    the round bodies (the arm-free minimum of a settled env is 4 corners + 1 + 2 end points; the median is well above what the cube alone gives)"""
    b, d, nc = _ragged("cpu", 1027)
    print("ragged: contacts median", np.median(nc[:, 0]), "max", nc[:, 0].max(), "refused", nc[:, 1].sum())
    assert np.isfinite(b).all() and int(nc[:, 1].sum()) == 0
    assert np.median(nc[:, 0]) >= 6 and nc[:, 0].max() <= 24


@pytest.mark.gpu
def test_scene_shapes_hip_matches_the_cpu_backend_on_every_env_of_a_ragged_batch():
    """the two product backends on the same 1027 mixed scenes (not a multiple of the kernel's envs per workgroup), 6 simulate() calls; limits of
    tests/test_scene.py: 99 % of the envs to 0.2 mm, none beyond 5 mm, the same contact count in > 97 % of the envs, no refusal"""
    n = 1027
    (bc, dc, nc), (bh, dh, nh) = _ragged("cpu", n), _ragged("cuda:0", n)
    assert np.isfinite(bh).all() and np.isfinite(dh).all()
    d = np.abs(bh - bc)
    d[..., 3:7] = np.minimum(d[..., 3:7], np.abs(bh[..., 3:7] + bc[..., 3:7]))
    per_env = d[..., :7].reshape(n, -1).max(axis=1)
    print("hip vs cpu: q99", np.quantile(per_env, 0.99), "max", per_env.max(), "dof", np.abs(dh[..., 0] - dc[..., 0]).max(), "same count", (nh[:, 0] == nc[:, 0]).mean())
    assert np.quantile(per_env, 0.99) < 2e-4 and per_env.max() < 5e-3, (np.quantile(per_env, 0.99), per_env.max())
    assert np.abs(dh[..., 0] - dc[..., 0]).max() < 2e-3
    assert (nh[:, 0] == nc[:, 0]).mean() > 0.97 and int(nh[:, 1].sum()) == int(nc[:, 1].sum()) == 0
    assert np.median(nh[:, 0]) >= 6
