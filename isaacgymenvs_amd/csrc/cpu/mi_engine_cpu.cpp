// mi_engine_cpu.cpp -- CPU product backend: the engine lifecycle part of include/mi_engine.h on a HOST arena.
//
// What it is for: the reference's `sim_device=cpu pipeline=cpu` configuration (BASELINE.json config 1: Cartpole num_envs=64;
// reference device resolution isaacgymenvs/tasks/base/vec_task.py:78-88, PhysX worker threads `num_threads`, cfg/config.yaml:30).
// What it is built from: the SAME sources the HIP kernels compile -- csrc/core/engine.hpp (per-env physics sub-step, host build of
// the specialised code), csrc/tasks/locomotion.hpp (observations / reward / reset), csrc/tasks/*_step.hpp (the per-env pre / post / reset /
// init bodies of Cartpole, Quadcopter, Ingenuity and BallBalance), csrc/arena_layout.hpp (arena layout) -- with OpenMP over envs where the
// kernels have one env per lane.  It does NOT use oracle/ (test infrastructure).  Same SoA arena layout,
// same counter-based reset RNG: the Python side sees identical tensors and, up to fp32 summation order in the episode statistics,
// identical numbers on both devices.
//
// Tasks: every task of the table (csrc/arena_layout.hpp).  This file: the C ABI + Cartpole, Ant, Humanoid (self-collision included), Quadcopter,
// Ingenuity, BallBalance; cpu_anymal.cpp: AnymalTerrain (BASELINE config 4), Anymal; cpu_hand.cpp + cpu_hand_physics.cpp: ShadowHand (config 5),
// AllegroHand.
// Build: g++ -fopenmp, one object per translation unit in parallel, linked into libmi_engine_cpu.so (isaacgymenvs_amd/native.py::build_cpu);
// the library exports the lifecycle subset of include/mi_engine.h.
#include "cpu_engine.hpp"
#include "cpu_hand.hpp"
#include "../core/bbot_engine.hpp"
#include "../tasks/quadcopter_step.hpp"
#include "../tasks/ingenuity_step.hpp"
#include "../tasks/ball_balance_step.hpp"

static thread_local std::string g_err;
static int fail(const std::string& m) { g_err = m; return -1; }
static int result(const std::string& err) { return err.empty() ? 0 : fail(err); }       // of a call into engine_core.hpp
extern "C" const char* mi_last_error(void) { return g_err.c_str(); }
extern "C" int mi_abi_version(void) { return MI_ABI_VERSION; }

extern "C" int mi_task_info(const char* task, MiTaskInfo* out) { return result(core_task_info(task, out)); }
extern "C" size_t mi_engine_arena_bytes(const char* task, int num_envs) {      // every task of the table has a host build
    const size_t n = core_arena_bytes(task, num_envs);
    if (n == 0) fail("mi_engine_arena_bytes: bad task or num_envs");
    return n;
}
extern "C" int mi_engine_create(const char* task, const MiSimParams* sim, const void* task_params, size_t task_params_bytes, int num_envs,
                                int env_id_offset, uint64_t seed, void* arena, size_t arena_bytes, MiEngine** out) {
    EngineCore core;
    if (int rc = result(core_create(core, task, sim, task_params, task_params_bytes, num_envs, env_id_offset, seed, arena, arena_bytes, out))) return rc;
    MiEngine* e = new (std::nothrow) MiEngine();
    if (!e) return fail("out of host memory");
    static_cast<EngineCore&>(*e) = core;
    e->num_threads = 4;   // cfg/config.yaml:30
    *out = e;
    return 0;
}
extern "C" void mi_engine_destroy(MiEngine* e) { delete e; }
extern "C" int mi_engine_num_tensors(const MiEngine* e) { return e ? (int)e->descs.size() : fail("null engine"); }
extern "C" int mi_engine_tensor_desc(const MiEngine* e, int i, MiTensorDesc* out) { return result(core_tensor_desc(e, i, out)); }

// the options only this library has, or answers in its own way (the others: engine_core.hpp kCoreOptions)
static const EngineOption kCpuOptions[] = {
    // GPU launch shapes: accepted, nothing to do here
    {"multi_wave", MI_ON_CPU, MI_SET { return {}; }, MI_GET { return 0; }},
    {"fused_sub", MI_ON_CPU, MI_SET { return {}; }, MI_GET { return 0; }},
    {"fused_post", MI_ON_CPU, MI_SET { return {}; }, MI_GET { return 0; }},
    {"dof_state_lag", MI_ON_CPU, MI_SET {
         return core_set_dof_state_lag(e, x, [&](size_t bytes) -> std::string { memcpy(e.dof_api_arena, e.v.dof, bytes); return {}; }); },
     core_get_dof_state_lag},
    // sim.physx.num_threads of the reference's CPU pipeline (vec_task.py:541, cfg/config.yaml:30): OpenMP threads over envs
    {"num_threads", MI_ON_CPU, MI_SET { if (x < 1) return "num_threads < 1"; static_cast<MiEngine&>(e).num_threads = (int)x; return {}; },
     MI_GET { return static_cast<const MiEngine&>(e).num_threads; }},
};
extern "C" int mi_engine_set_option(MiEngine* e, const char* key, double value) { return result(core_set_option(e, key, value, MI_ON_CPU, kCpuOptions)); }
extern "C" int mi_engine_get_option(const MiEngine* e, const char* key, double* out) { return result(core_get_option(e, key, out, MI_ON_CPU, kCpuOptions)); }
extern "C" int mi_engine_set_noise(MiEngine* e, int which, const MiNoiseParams* p) { return result(core_set_noise(e, which, p)); }
extern "C" int mi_engine_last_ring(const MiEngine* e) { return core_last_ring(e); }
// the terrain arrays are copied: the engine does not depend on the caller keeping its buffers alive
extern "C" int mi_engine_set_terrain(MiEngine* e, const int16_t* height_samples, int rows, int cols, float horizontal_scale, float vertical_scale,
                                     float border_size, const float* env_origins, int num_levels, int num_terrains, float env_length, int max_init_level) {
    if (int rc = result(core_check_terrain_args(e, height_samples, rows, cols, horizontal_scale, env_origins, num_levels, num_terrains))) return rc;
    e->terrain_hs.assign(height_samples, height_samples + (size_t)rows * cols);
    e->terrain_origins.assign(env_origins, env_origins + (size_t)num_levels * num_terrains * 3);
    core_set_terrain(*e, e->terrain_hs.data(), rows, cols, horizontal_scale, vertical_scale, border_size, e->terrain_origins.data(), num_levels, num_terrains,
                     env_length, max_init_level);
    return 0;
}
extern "C" int mi_engine_set_scene_statics(MiEngine* e, int n, const float* pos, const float* quat, const float* half, const float* mu) {
    return result(core_set_scene_statics(e, n, pos, quat, half, mu));
}
static int hand_call(MiEngine* e, int what, const float* actions, bool simulate_only, const int64_t* ids, int n, float* out_j, float* out_h) {
    const bool sh = e->task == T_SHADOWHAND;
    switch (what) {
        case 0: return sh ? cpu_hand0_init(e) : cpu_hand1_init(e);
        case 1: return sh ? cpu_hand0_step(e, actions, simulate_only) : cpu_hand1_step(e, actions, simulate_only);
        case 2: return sh ? cpu_hand0_reset(e, ids, n) : cpu_hand1_reset(e, ids, n);
        case 3: return sh ? cpu_hand0_body_states(e) : cpu_hand1_body_states(e);
        default: return sh ? cpu_hand0_kinematics(e, out_j, out_h) : cpu_hand1_kinematics(e, out_j, out_h);
    }
}

// ------------------------------------------------------------------------------------------------ initial state (= init_state_kernel)
extern "C" int mi_engine_init_state(MiEngine* e, void*) {
    if (!e) return fail("null engine");
    const TaskMeta& m = kTasks[e->task];
    const int N = e->N;
    if (is_hand_task(e->task)) {
        e->steps = 0;
        const int rc = hand_call(e, 0, nullptr, false, nullptr, 0, nullptr, nullptr);
        return rc == -2 ? fail("mi_engine_init_state: the hand model of this library and its task table have different sizes (a variant built without its engine unit)") : rc;
    }
    if (e->task == T_ANYMAL && e->terrain.hs == nullptr) return fail("mi_engine_init_state: AnymalTerrain needs mi_engine_set_terrain first");
    const View v0 = init_view(*e);
    for (int en = 0; en < N; ++en)
        init_env_constants(v0, en, m.nd, 3 * m.nsph, 6 * m.nsens, m.nobs, m.nact, core_init_root_z(*e), core_is_loco(*e) ? e->loco.initial_dof_pos : nullptr, core_init_potential(*e));
    for (int en = 0; en < N; ++en) {      // the tasks' own tensors
        if (e->task == T_QUADCOPTER) quad_init_env(e->v, e->qv, e->quad, en);
        else if (e->task == T_INGENUITY) ing_init_env(e->v, e->iv, e->ing, en);
        else if (e->task == T_BALLBALANCE) bbot_init_env(e->v, e->bv, e->bbot, en);
    }
    e->steps = 0;
    if (e->task == T_ANYMAL || e->task == T_ANYMAL_FLAT) {
        std::string err;
        if (cpu_anymal_init(e, &err) != 0) return fail(err);
    }
    if (e->task == T_ARTICULATION) cpu_articulation_reset(e, nullptr, 0);
    return 0;
}

// ------------------------------------------------------------------------------------------------ one env on the host
template <class M>
static inline void load_env(Sim<M>& s, const View& v, int en) {
    const int N = v.N;
    for (int k = 0; k < 13; ++k) s.root[k] = v.root[k * N + en];
    for (int k = 0; k < M::ND; ++k) { s.q[k] = v.dof[k * N + en]; s.qd[k] = v.dof[(M::ND + k) * N + en]; }
}
template <class M>
static inline void store_env(const Sim<M>& s, const View& v, int en) {
    const int N = v.N;
    for (int k = 0; k < 13; ++k) v.root[k * N + en] = s.root[k];
    for (int k = 0; k < M::ND; ++k) { v.dof[k * N + en] = s.q[k]; v.dof[(M::ND + k) * N + en] = s.qd[k]; }
}
// gym.simulate(): `substeps` sub-steps with the efforts in tau (what substep_kernel does per lane)
template <class M>
static void simulate_env(const View& v, const SimParams& P, int en, const float* tau) {
    if constexpr (M::ACTOR_SCALES != 0 && !is_scaled<M>::value) {
        // option actor_tensors: the instantiation that reads the `actor_params` factors, as on the device (step_kernels.hpp launch_substeps)
        if (v.actor_scale != nullptr || v.limit_shift != nullptr) return simulate_env<Scaled<M>>(v, P, en, tau);
    }
    const int N = v.N;
    Sim<M> sim;
    load_env(sim, v, en);
    if constexpr (Sim<M>::SCALED) {
        if (v.actor_scale) sim.actor_scale = Strided{v.actor_scale + en, N};
        if (v.limit_shift) sim.limit_shift = Strided{v.limit_shift + en, N};
    }
    const float h = P.dt / (float)P.substeps;
    float rows[Sim<M>::ROW_SLOTS > 0 ? Sim<M>::ROW_SLOTS : 1];
    const SelfCol sc{Strided{v.lamp ? v.lamp + en : nullptr, N}, Strided{v.pairf ? v.pairf + en : nullptr, N}, v.dropped ? v.dropped + en : nullptr, N};
    const float mu_env = v.friction ? v.friction[en] : -1.f;
    for (int ss = 0; ss < P.substeps; ++ss)
        sim.substep(P, tau, h, RowStore<1>{rows}, Strided{v.lamc + en, N}, Strided{v.laml + en, N}, Strided{v.sensor + en, N},
                    Strided{v.dof_force + en, N}, PlaneGround{}, mu_env, Strided{nullptr, N}, nullptr, false,
                    (Sim<M>::NPG > 0 && v.lamp) ? &sc : nullptr);
    store_env(sim, v, en);
}
// post_physics_step of Ant / Humanoid for one env (what loco_post_kernel does per lane; reference ant.py:287-297)
template <class M, bool HUM>
static void loco_post_env(const View& v, const LocoParams& tp, int en, StatAcc& acc) {
    using T = Loco<M::ND, 6 * M::NSENS, HUM>;
    constexpr int ND = M::ND, NOBS = T::NOBS;
    const int N = v.N;
    float root[13], q[ND], qd[ND], dof_force[ND], sensor[6 * M::NSENS > 0 ? 6 * M::NSENS : 1], act[ND];
    for (int k = 0; k < 13; ++k) root[k] = v.root[k * N + en];
    for (int k = 0; k < ND; ++k) {
        q[k] = v.dof[k * N + en]; qd[k] = v.dof[(ND + k) * N + en];
        dof_force[k] = v.dof_force[k * N + en]; act[k] = v.actions[k * N + en];
    }
    for (int k = 0; k < 6 * M::NSENS; ++k) sensor[k] = v.sensor[k * N + en];
    long long progress = v.progress[en] + 1;
    float potentials = v.potentials[en], prev_potentials;
    int ep = v.episode[en];
    if (v.reset[en] != 0) {
        float init_root[13];
        for (int k = 0; k < 13; ++k) init_root[k] = v.init_root[k * N + en];
        T::reset(tp, v.seed, (uint32_t)(v.env_offset + en), (uint32_t)ep, init_root, root, q, qd, &potentials, &prev_potentials);
        ep += 1;
        progress = 0;
        for (int k = 0; k < 13; ++k) v.root[k * N + en] = root[k];
        for (int k = 0; k < ND; ++k) { v.dof[k * N + en] = q[k]; v.dof[(ND + k) * N + en] = qd[k]; v.laml[k * N + en] = 0.f; }
        for (int k = 0; k < 3 * M::NSPH; ++k) v.lamc[k * N + en] = 0.f;
        if (M::NPG > 0 && v.lamp) for (int k = 0; k < 3 * M::NPG; ++k) v.lamp[k * N + en] = 0.f;
    }
    float obs[NOBS], up_vec[3], heading_vec[3];
    T::observations(tp, root, tp.targets, potentials, tp.inv_start_rot, q, qd, dof_force, tp.dof_lower, tp.dof_upper, sensor, act,
                    tp.basis_vec0, tp.basis_vec1, obs, &potentials, &prev_potentials, up_vec, heading_vec);
    float rew;
    long long reset;
    T::reward(tp, obs, 0LL, progress, act, potentials, prev_potentials, &rew, &reset);
    if (v.obs_noise.dist != 0)
        for (int k = 0; k < NOBS; ++k) obs[k] = apply_noise(v.obs_noise, v.seed, (uint32_t)(v.env_offset + en), v.step, 0u, (uint32_t)k, obs[k]);
    episode_stats_env(v, en, rew, reset, progress, acc);
    v.episode[en] = ep;
    v.potentials[en] = potentials; v.prev_potentials[en] = prev_potentials;
    for (int k = 0; k < 3; ++k) { v.up_vec[k * N + en] = up_vec[k]; v.heading_vec[k * N + en] = heading_vec[k]; }
    store_step_outputs(v, en, obs, rew, reset, progress, tp.max_episode_length);
}
template <class M>
static void load_tau(const View& v, int en, float* tau) { for (int k = 0; k < M::ND; ++k) tau[k] = v.tau[k * v.N + en]; }

// VecTask.step for one env: clamp -> efforts (pre_physics_step) -> control_freq_inv x simulate -> post_physics_step
template <class M, bool HUM>
static void step_loco(MiEngine* e, const float* actions) {
    const View& v = e->v;
    const int N = v.N;
    const LocoParams& tp = e->loco;
    std::vector<StatAcc> accs(e->num_threads);
#pragma omp parallel for schedule(static) num_threads(e->num_threads)
    for (int en = 0; en < N; ++en) {
        float tau[M::NDA];
        for (int k = 0; k < M::ND; ++k) {
            float a = actions[(size_t)en * M::ND + k];
            if (v.act_noise.dist != 0) a = apply_noise(v.act_noise, v.seed, (uint32_t)(v.env_offset + en), v.step, 1u, (uint32_t)k, a);
            a = fminf(fmaxf(a, -tp.clip_actions), tp.clip_actions);                                             // vec_task.py:374
            v.actions[k * N + en] = a;
            tau[k] = a * tp.gear[k] * tp.power_scale;                                                            // ant.py:281-285
            v.tau[k * N + en] = tau[k];
        }
        for (int c = 0; c < e->control_freq_inv; ++c) simulate_env<M>(v, e->P, en, tau);
        loco_post_env<M, HUM>(v, tp, en, accs[omp_get_thread_num()]);
    }
    flush_stats(v, accs);
}
static void step_cartpole(MiEngine* e, const float* actions) {
    using M = ModelCartpole;
    const View& v = e->v;
    const int N = v.N;
    const CartpoleParams& tp = e->cart;
    std::vector<StatAcc> accs(e->num_threads);
#pragma omp parallel for schedule(static) num_threads(e->num_threads)
    for (int en = 0; en < N; ++en) {
        float tau[M::NDA];
        float a = actions[en];
        if (v.act_noise.dist != 0) a = apply_noise(v.act_noise, v.seed, (uint32_t)(v.env_offset + en), v.step, 1u, 0u, a);
        a = fminf(fmaxf(a, -tp.clip_actions), tp.clip_actions);
        v.actions[en] = a;
        tau[0] = a * tp.max_push_effort; tau[1] = 0.f;            // cartpole.py:159-163: effort on DoF 0 only
        v.tau[en] = tau[0]; v.tau[N + en] = 0.f;
        for (int c = 0; c < e->control_freq_inv; ++c) simulate_env<M>(v, e->P, en, tau);
        cartpole_post_env(v, tp, en, HostEpisodeRed{&accs[omp_get_thread_num()]});
    }
    flush_stats(v, accs);
}

// ---- the small tasks: pre_physics_step, post_physics_step and the resets are the bodies of tasks/*_step.hpp that the kernels run; the
// sub-steps between them are this file's own (a stack row store where the kernels use LDS)
static inline void clamp_angular_speed(float* root, float lim) {      // asset_options.max_angular_velocity
    const float w2 = root[10] * root[10] + root[11] * root[11] + root[12] * root[12];
    if (w2 > lim * lim) { const float sc = lim / sqrtf(w2); root[10] *= sc; root[11] *= sc; root[12] *= sc; }
}
template <class M, int NR>
static void drive_substeps(const View& v, const SimParams& P, int en, int n_sub, float kp, float kd, const float* target, const float* fs, float wmax) {
    const int N = v.N;
    Sim<M> sim;
    load_env(sim, v, en);
    float tau[M::NDA] = {0}, rows[Sim<M>::ROW_SLOTS > 0 ? Sim<M>::ROW_SLOTS : 1];
    const Drive drv{kp, kd, target, fs};
    const float h = P.dt / (float)P.substeps;
    for (int ss = 0; ss < n_sub; ++ss) {
        sim.substep(P, tau, h, RowStore<1>{rows}, Strided{v.lamc + en, N}, Strided{v.laml + en, N}, Strided{v.sensor + en, N},
                    Strided{v.dof_force + en, N}, PlaneGround{}, -1.f, Strided{nullptr, N}, &drv);
        clamp_angular_speed(sim.root, wmax);
    }
    store_env(sim, v, en);
}
static void step_quadcopter(MiEngine* e, const float* actions, bool simulate_only) {
    using QM = ModelQuadcopter;
    const View& v = e->v;
    const QuadView& qv = e->qv;
    const QuadcopterParams& p = e->quad;
    const int N = v.N;
    std::vector<StatAcc> accs(e->num_threads);
#pragma omp parallel for schedule(static) num_threads(e->num_threads)
    for (int en = 0; en < N; ++en) {
        if (!simulate_only) quad_pre_env(v, qv, p, actions, en);
        float target[kQuadDof], fs[kQuadRotors][3];
        for (int d = 0; d < kQuadDof; ++d) target[d] = qv.targets[d * N + en];
        for (int k = 0; k < kQuadRotors; ++k) { fs[k][0] = fs[k][1] = 0.f; fs[k][2] = qv.forces[(3 * QM::sens_body[k] + 2) * N + en]; }
        drive_substeps<QM, kQuadRotors>(v, e->P, en, (simulate_only ? 1 : e->control_freq_inv) * e->P.substeps, p.drive_stiffness, p.drive_damping, target, &fs[0][0], p.max_angular_velocity);
        if (!simulate_only) quad_post_env(v, qv, p, en, HostEpisodeRed{&accs[omp_get_thread_num()]});
    }
    flush_stats(v, accs);
}
static void step_ingenuity(MiEngine* e, const float* actions, bool simulate_only) {
    using IM = ModelIngenuity;
    const View& v = e->v;
    const IngenuityView& iv = e->iv;
    const IngenuityParams& p = e->ing;
    const int N = v.N;
    std::vector<StatAcc> accs(e->num_threads);
#pragma omp parallel for schedule(static) num_threads(e->num_threads)
    for (int en = 0; en < N; ++en) {
        if (!simulate_only) ing_pre_env(v, iv, p, actions, en);
        float target[kIngDof] = {0}, fs[kIngRotors][3];
        for (int r = 0; r < kIngRotors; ++r) for (int k = 0; k < 3; ++k) fs[r][k] = iv.forces[(3 * IM::sens_body[r] + k) * N + en];
        drive_substeps<IM, kIngRotors>(v, e->P, en, (simulate_only ? 1 : e->control_freq_inv) * e->P.substeps, 0.f, 0.f, target, &fs[0][0], p.max_angular_velocity);
        if (!simulate_only) ing_post_env(v, iv, p, en, HostEpisodeRed{&accs[omp_get_thread_num()]});
    }
    flush_stats(v, accs);
}
static void step_ball_balance(MiEngine* e, const float* actions, bool simulate_only) {
    using BM = ModelBalanceBot;
    const View& v = e->v;
    const BbotView& bv = e->bv;
    const BallBalanceParams& p = e->bbot;
    const BbotPhys& ph = *reinterpret_cast<const BbotPhys*>(&p.pin_stiffness);
    static_assert(sizeof(BbotPhys) == sizeof(BallBalanceParams) - offsetof(BallBalanceParams, pin_stiffness), "BbotPhys is the tail of BallBalanceParams");
    const int N = v.N;
    std::vector<StatAcc> accs(e->num_threads);
#pragma omp parallel for schedule(static) num_threads(e->num_threads)
    for (int en = 0; en < N; ++en) {
        if (!simulate_only) bbot_pre_env(v, bv, p, actions, en);
        BbotSim<BM> sim;
        load_env(sim, v, en);
        float target[kBbotDof];
        for (int d = 0; d < kBbotDof; ++d) target[d] = bv.targets[d * N + en];
        for (int k = 0; k < 3; ++k) { sim.ball.pos[k] = bv.ball[k * N + en]; sim.ball.vel[k] = bv.ball[(7 + k) * N + en]; sim.ball.angvel[k] = bv.ball[(10 + k) * N + en]; }
        for (int k = 0; k < 4; ++k) sim.ball.quat[k] = bv.ball[(3 + k) * N + en];
        int nc = 0;
        const int n_sub = (simulate_only ? 1 : e->control_freq_inv) * e->P.substeps;
        for (int ss = 0; ss < n_sub; ++ss)
            sim.substep(e->P, ph, e->P.dt / (float)e->P.substeps, target, Strided{v.laml + en, N}, Strided{bv.lamp + en, N}, Strided{v.sensor + en, N}, &nc);
        bv.ncontact[en] = nc;
        store_env(sim, v, en);
        for (int k = 0; k < 3; ++k) { bv.ball[k * N + en] = sim.ball.pos[k]; bv.ball[(7 + k) * N + en] = sim.ball.vel[k]; bv.ball[(10 + k) * N + en] = sim.ball.angvel[k]; }
        for (int k = 0; k < 4; ++k) bv.ball[(3 + k) * N + en] = sim.ball.quat[k];
        if (!simulate_only) bbot_post_env(v, bv, p, en, HostEpisodeRed{&accs[omp_get_thread_num()]});
    }
    flush_stats(v, accs);
}

extern "C" int mi_engine_step(MiEngine* e, const float* actions, void*) {
    if (!e || !actions) return fail("mi_engine_step: null argument");
    e->v.ring = (int)(e->steps & 1);
    e->v.step = (unsigned)e->steps;
    switch (e->task) {
        case T_CARTPOLE: step_cartpole(e, actions); break;
        case T_ANT: step_loco<ModelAnt, false>(e, actions); break;
        case T_HUMANOID: step_loco<ModelHumanoid, true>(e, actions); break;
        case T_QUADCOPTER: step_quadcopter(e, actions, false); break;
        case T_INGENUITY: step_ingenuity(e, actions, false); break;
        case T_BALLBALANCE: step_ball_balance(e, actions, false); break;
        case T_ANYMAL:
            if (e->terrain.hs == nullptr) return fail("mi_engine_step: AnymalTerrain needs mi_engine_set_terrain first");
            cpu_anymal_step(e, actions, false);
            break;
        case T_ANYMAL_FLAT: cpu_anymal_step(e, actions, false); break;
        case T_SHADOWHAND: case T_ALLEGROHAND: hand_call(e, 1, actions, false, nullptr, 0, nullptr, nullptr); break;
        case T_ARTICULATION: return fail("mi_engine_step: the Articulation task has no task kernels -- drive it with mi_engine_simulate (gym.simulate) and keep "
                                         "the observation / reward code on the caller's side");
        default: return fail("mi_engine_step: task not on the CPU backend");
    }
    e->steps++;
    return 0;
}
template <class M>
static void simulate_all(MiEngine* e) {
    const View& v = e->v;
#pragma omp parallel for schedule(static) num_threads(e->num_threads)
    for (int en = 0; en < v.N; ++en) {
        float tau[M::NDA];
        load_tau<M>(v, en, tau);
        simulate_env<M>(v, e->P, en, tau);
    }
}
extern "C" int mi_engine_simulate(MiEngine* e, void*) {
    if (!e) return fail("null engine");
    switch (e->task) {
        case T_CARTPOLE: simulate_all<ModelCartpole>(e); break;
        case T_ANT: simulate_all<ModelAnt>(e); break;
        case T_HUMANOID: simulate_all<ModelHumanoid>(e); break;
        case T_QUADCOPTER: step_quadcopter(e, nullptr, true); break;
        case T_INGENUITY: step_ingenuity(e, nullptr, true); break;
        case T_BALLBALANCE: step_ball_balance(e, nullptr, true); break;
        case T_ANYMAL:
            if (e->terrain.hs == nullptr) return fail("mi_engine_simulate: AnymalTerrain needs mi_engine_set_terrain first");
            cpu_anymal_step(e, nullptr, true);
            break;
        case T_ANYMAL_FLAT: cpu_anymal_step(e, nullptr, true); break;
        case T_SHADOWHAND: case T_ALLEGROHAND: hand_call(e, 1, nullptr, true, nullptr, 0, nullptr, nullptr); break;
        case T_ARTICULATION: cpu_articulation_simulate(e); break;
        default: return fail("mi_engine_simulate: task not on the CPU backend");
    }
    return 0;
}
// gym.refresh_rigid_body_state_tensor: Sim<M>::body_state for every (env, body)
template <class M>
static void body_states_all(MiEngine* e) {
    const View& v = e->v;
    const int N = v.N;
#pragma omp parallel for schedule(static) num_threads(e->num_threads)
    for (int en = 0; en < N; ++en) {
        Sim<M> sim;
        load_env(sim, v, en);
        sfor<M::NB>([&](auto B_) {
            constexpr int b = decltype(B_)::value;
            float o[13];
            sim.template body_state<b>(o);
            for (int k = 0; k < 13; ++k) v.body_state[(b * 13 + k) * N + en] = o[k];
        });
    }
}
extern "C" int mi_engine_refresh_rigid_body_states(MiEngine* e, void*) {
    if (!e) return fail("null engine");
    switch (e->task) {
        case T_CARTPOLE: body_states_all<ModelCartpole>(e); break;
        case T_ANT: body_states_all<ModelAnt>(e); break;
        case T_HUMANOID: body_states_all<ModelHumanoid>(e); break;
        case T_QUADCOPTER: body_states_all<ModelQuadcopter>(e); break;
        case T_INGENUITY: body_states_all<ModelIngenuity>(e); break;
        case T_BALLBALANCE: body_states_all<ModelBalanceBot>(e); break;
        case T_ANYMAL: case T_ANYMAL_FLAT: cpu_anymal_body_states(e); break;
        case T_SHADOWHAND: case T_ALLEGROHAND: hand_call(e, 3, nullptr, false, nullptr, 0, nullptr, nullptr); break;
        case T_ARTICULATION: cpu_articulation_body_states(e); break;
        default: return fail("mi_engine_refresh_rigid_body_states: task not on the CPU backend");
    }
    return 0;
}
// gym.refresh_jacobian_tensors / refresh_mass_matrix_tensors into caller tensors (csrc/kernels_body_states.hip on the device)
template <class M>
static void kinematics_views_all(MiEngine* e, float* out_j, float* out_h) {
    const View& v = e->v;
    const int N = v.N;
    constexpr int NV = M::NV;
#pragma omp parallel for schedule(static)
    for (int en = 0; en < N; ++en) {
        Sim<M> sim;
        load_env(sim, v, en);
        if (out_j) {
            sfor<M::NB>([&](auto B_) {
                constexpr int b = decltype(B_)::value;
                sim.template body_jacobian<b>(out_j + ((size_t)en * M::NB + b) * 6 * NV);
            });
        }
        if (out_h) sim.mass_matrix(e->P, out_h + (size_t)en * NV * NV);
    }
}
static int kinematics_views(MiEngine* e, float* out_j, float* out_h, const char* who) {
    if (!e || (!out_j && !out_h)) return fail(std::string(who) + ": null argument");
    switch (e->task) {
        case T_CARTPOLE: kinematics_views_all<ModelCartpole>(e, out_j, out_h); break;
        case T_ANT: kinematics_views_all<ModelAnt>(e, out_j, out_h); break;
        case T_HUMANOID: kinematics_views_all<ModelHumanoid>(e, out_j, out_h); break;
        case T_QUADCOPTER: kinematics_views_all<ModelQuadcopter>(e, out_j, out_h); break;
        case T_INGENUITY: kinematics_views_all<ModelIngenuity>(e, out_j, out_h); break;
        case T_BALLBALANCE: kinematics_views_all<ModelBalanceBot>(e, out_j, out_h); break;
        case T_ANYMAL: case T_ANYMAL_FLAT: cpu_anymal_kinematics(e, out_j, out_h); break;
        case T_SHADOWHAND: case T_ALLEGROHAND: hand_call(e, 4, nullptr, false, nullptr, 0, out_j, out_h); break;
        case T_ARTICULATION: cpu_articulation_kinematics(e, out_j, out_h); break;
        default: return fail(std::string(who) + ": task not on the CPU backend");
    }
    return 0;
}
extern "C" int mi_engine_compute_jacobians(MiEngine* e, float* out, void*) { return kinematics_views(e, out, nullptr, "mi_engine_compute_jacobians"); }
extern "C" int mi_engine_compute_mass_matrices(MiEngine* e, float* out, void*) { return kinematics_views(e, nullptr, out, "mi_engine_compute_mass_matrices"); }

// reset_idx(env_ids): ids outside the batch are skipped, a repeated id resets again (the next episode's draws)
template <class F>
static void for_env_ids(const View& v, const int64_t* ids, int n, F reset_env) {
    for (int i = 0; i < n; ++i) if (ids[i] >= 0 && ids[i] < v.N) reset_env((int)ids[i]);
}
extern "C" int mi_engine_reset_idx(MiEngine* e, const int64_t* env_ids, int n, void*) {
    if (!e) return fail("null engine");
    if (n <= 0) return 0;
    if (!env_ids) return fail("mi_engine_reset_idx: null env_ids");
    const View& v = e->v;
    switch (e->task) {
        case T_CARTPOLE: for_env_ids(v, env_ids, n, [&](int en) { cartpole_reset_env(v, en); }); break;
        case T_ANT: for_env_ids(v, env_ids, n, [&](int en) { loco_reset_env<ModelAnt, false>(v, e->loco, en); }); break;
        case T_HUMANOID: for_env_ids(v, env_ids, n, [&](int en) { loco_reset_env<ModelHumanoid, true>(v, e->loco, en); }); break;
        case T_QUADCOPTER: for_env_ids(v, env_ids, n, [&](int en) { float q[kQuadDof]; quad_reset_env(v, e->qv, e->quad, en, q); }); break;
        case T_INGENUITY: for_env_ids(v, env_ids, n, [&](int en) { ing_reset_env(v, e->iv, e->ing, en, v.episode[en]); }); break;
        case T_BALLBALANCE:
            for_env_ids(v, env_ids, n, [&](int en) {
                bbot_reset_env(v, e->bv, e->bbot, en);
                for (int d = 0; d < kBbotDof; ++d) e->bv.targets[d * v.N + en] = 0.f;          // the pre step's `rs ? 0 : t`
            });
            break;
        case T_ANYMAL: case T_ANYMAL_FLAT: cpu_anymal_reset(e, env_ids, n); break;
        case T_SHADOWHAND: case T_ALLEGROHAND: hand_call(e, 2, nullptr, false, env_ids, n, nullptr, nullptr); break;
        case T_ARTICULATION: cpu_articulation_reset(e, env_ids, n); break;
        default: return fail("mi_engine_reset_idx: task not on the CPU backend");
    }
    return 0;
}
