// engine_core.hpp -- the engine lifecycle of include/mi_engine.h that touches no device: task table queries, the checks and the layout of
// mi_engine_create, the option table, noise, terrain arguments, the per-env constants of the initial state.  One definition for the HIP library
// (mi_engine.hip) and the CPU backend (cpu/mi_engine_cpu.cpp): their extern "C" entry points are thin calls into this file, and each keeps its own
// thread_local error string.  Host code only: no HIP header, no kernel, and not the run-time robot's header (gen/model_articulation.h).
// A function that can refuse returns the error text, empty when all is well.
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_engine.h"
#include "arena_layout.hpp"
#include "task_views.hpp"
#include "tasks/shadow_hand.hpp"
#include "tasks/articulation.hpp"

static_assert(sizeof(MiSimParams) == sizeof(SimParams), "MiSimParams layout");
static_assert(sizeof(MiLocoParams) == sizeof(LocoParams), "MiLocoParams layout");
static_assert(sizeof(MiCartpoleParams) == sizeof(CartpoleParams), "MiCartpoleParams layout");
static_assert(MI_MAX_DOF == mi::kMaxDof, "MI_MAX_DOF");
static_assert(sizeof(MiAnymalParams) == sizeof(AnymalParams), "MiAnymalParams layout");
static_assert(sizeof(MiAnymalFlatParams) == sizeof(AnymalFlatParams), "MiAnymalFlatParams layout");
static_assert(sizeof(MiQuadcopterParams) == sizeof(QuadcopterParams), "MiQuadcopterParams layout");
static_assert(sizeof(MiIngenuityParams) == sizeof(IngenuityParams), "MiIngenuityParams layout");
static_assert(sizeof(MiBallBalanceParams) == sizeof(BallBalanceParams), "MiBallBalanceParams layout");
static_assert(sizeof(MiHandRewardParams) == sizeof(HandRewardParams), "MiHandRewardParams layout");
static_assert(sizeof(MiHandParams) == sizeof(HandParams), "MiHandParams layout");
static_assert(sizeof(MiArticulationParams) == sizeof(ArticulationParams), "MiArticulationParams layout");
static_assert(sizeof(MiNoiseParams) == sizeof(NoiseParams), "MiNoiseParams layout");

// what both libraries' `struct MiEngine` start with (HIP adds its device, the CPU backend its threads and its copy of the terrain)
struct EngineCore {
    int task, N;
    SimParams P;
    LocoParams loco;
    CartpoleParams cart;
    AnymalParams anymal;
    AnymalFlatParams anymal_flat;
    QuadcopterParams quad;
    QuadView qv;
    IngenuityParams ing;
    IngenuityView iv;
    BallBalanceParams bbot;
    BbotView bv;
    AnymalTerrainDesc terrain;
    HandParams hand;
    HandView hv;
    ArticulationParams artic;
    SceneStatics statics;   // the Articulation scene's static boxes as a wide-capacity library reads them (mi_engine_set_scene_statics; default: artic.scene's)
    int max_init_level;
    View v;
    float clip_obs;
    int control_freq_inv;
    std::vector<MiTensorDesc> descs;
    unsigned long long steps;
    // the `actor_params` tensors (actor_scale, dof_limit_shift) of Ant / Humanoid: the sub-step only reads them once the option
    // "actor_tensors" is on -- with the option off (default) it runs on the model's constants and skips the loads
    float* actor_scale_arena;
    float* limit_shift_arena;
    float* lamp_arena;     // the self-contact impulse tensor (Humanoid), kept while the option self_collision is 0
    float* dof_api_arena;  // the refreshed dof-state tensor (AnymalTerrain), kept while the option dof_state_lag is 0
};

inline std::string core_task_info(const char* task, MiTaskInfo* out) {
    const int t = task ? find_task(task) : -1;
    if (t < 0 || !out) return std::string("unknown task: ") + (task ? task : "(null)");
    const TaskMeta& m = kTasks[t];
    out->num_obs = m.nobs; out->num_actions = m.nact; out->num_dofs = m.nd; out->num_bodies = m.nb;
    out->num_sensors = m.nsens; out->num_contact_spheres = m.nsph; out->fixed_base = m.fixed;
    out->task_params_bytes = (int)m.pbytes;
    return {};
}

// the task's own tensors behind the common ones; e == nullptr: sizes only
inline void core_task_layout(int t, int n, Layout& L, EngineCore* e, char* base) {
    if (is_hand_task(t)) build_hand_layout(t, n, L, e ? &e->hv : nullptr, base);
    if (t == T_QUADCOPTER) build_quad_layout(n, L, e ? &e->qv : nullptr, base);
    if (t == T_INGENUITY) build_ingenuity_layout(n, L, e ? &e->iv : nullptr, base);
    if (t == T_BALLBALANCE) build_bbot_layout(n, L, e ? &e->bv : nullptr, base);
}
// 0: unknown task or num_envs <= 0 (a narrower ShadowHand observationType only uses a prefix of obs_buf / obs_out)
inline size_t core_arena_bytes(const char* task, int num_envs) {
    const int t = task ? find_task(task) : -1;
    if (t < 0 || num_envs <= 0) return 0;
    Layout L;
    build_layout(t, num_envs, L, nullptr, nullptr);
    core_task_layout(t, num_envs, L, nullptr, nullptr);
    return L.off;
}

// the engine's static set as mi_engine_create leaves it: MiScene.static_* (at most MI_SCENE_MAX_STATIC boxes)
inline void core_default_statics(EngineCore& e) {
    const SceneParams& sc = e.artic.scene;
    e.statics = SceneStatics{};
    e.statics.n = sc.n_static < 0 ? 0 : (sc.n_static < kSceneMaxStatic ? sc.n_static : kSceneMaxStatic);
    for (int i = 0; i < e.statics.n; ++i) {
        for (int k = 0; k < 3; ++k) { e.statics.pos[i][k] = sc.static_pos[i][k]; e.statics.half[i][k] = sc.static_half[i][k]; }
        for (int k = 0; k < 4; ++k) e.statics.quat[i][k] = sc.static_quat[i][k];
        e.statics.mu[i] = sc.static_mu[i];
    }
}
// static boxes the scene form of this library's Articulation unit holds (MI_SCENE_MAX_STATIC, or MI_SCENE_MAX_STATIC_WIDE for a variant built wide)
inline int core_scene_static_capacity() { const int c = mi_articulation_meta().static_cap; return c > 0 ? c : kSceneMaxStatic; }
// mi_engine_set_scene_statics: replaces the engine's whole static set.  Host only: the next sub-step launch carries the new set.  The first
// MI_SCENE_MAX_STATIC boxes are mirrored into artic.scene (what a capacity-4 library simulates, and what anything that reads MiScene sees).
inline std::string core_set_scene_statics(EngineCore* e, int n, const float* pos, const float* quat, const float* half, const float* mu) {
    if (!e) return "null engine";
    if (e->task != T_ARTICULATION || !mi_articulation_meta().fixed)
        return "mi_engine_set_scene_statics: only a fixed-base Articulation engine has a scene";
    const int cap = core_scene_static_capacity();
    if (n < 0) return "mi_engine_set_scene_statics: n < 0";
    if (n > cap) return "mi_engine_set_scene_statics: " + std::to_string(n) + " static boxes, this library's scene holds " + std::to_string(cap) +
                        " (capacity " + std::to_string(MI_SCENE_MAX_STATIC_WIDE) + ": a variant built with MI_SCENE_STATIC_CAP=" + std::to_string(MI_SCENE_MAX_STATIC_WIDE) + ")";
    if (n > 0 && (!pos || !quat || !half || !mu)) return "mi_engine_set_scene_statics: null array with n > 0";
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k)
            if (!(half[3 * i + k] > 0.f)) return "mi_engine_set_scene_statics: static box " + std::to_string(i) + " has a non-positive half size";
        double q2 = 0;
        for (int k = 0; k < 4; ++k) q2 += (double)quat[4 * i + k] * quat[4 * i + k];
        if (!(std::fabs(std::sqrt(q2) - 1.0) <= 1e-3)) return "mi_engine_set_scene_statics: static box " + std::to_string(i) + " has a quaternion that is not of unit norm";
    }
    SceneStatics st{};
    st.n = n;
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) { st.pos[i][k] = pos[3 * i + k]; st.half[i][k] = half[3 * i + k]; }
        for (int k = 0; k < 4; ++k) st.quat[i][k] = quat[4 * i + k];
        st.mu[i] = mu[i];
    }
    e->statics = st;
    SceneParams& sc = e->artic.scene;
    sc.n_static = n < kSceneMaxStatic ? n : kSceneMaxStatic;
    for (int i = 0; i < kSceneMaxStatic; ++i) {
        for (int k = 0; k < 3; ++k) { sc.static_pos[i][k] = i < n ? st.pos[i][k] : 0.f; sc.static_half[i][k] = i < n ? st.half[i][k] : 0.f; }
        for (int k = 0; k < 4; ++k) sc.static_quat[i][k] = i < n ? st.quat[i][k] : 0.f;
        sc.static_mu[i] = i < n ? st.mu[i] : 0.f;
    }
    return {};
}

inline const char* core_check_hand(int t, const HandParams& hp) {
    const int nfull = kTasks[t].nobs;     // ShadowHand 211, AllegroHand 88
    const bool ok = (hp.obs_type == 0 && hp.num_obs == nfull) || (hp.obs_type >= 1 && hp.obs_type <= 3 && hp.num_obs >= 1 && hp.num_obs <= 160);
    if (!ok) return "mi_engine_create: hand task obs_type / num_obs invalid";
    if (hp.object_shape < 0 || hp.object_shape > 2) return "mi_engine_create: hand task object_shape must be 0 (block), 1 (pen) or 2 (egg)";
    if (hp.object_shape != 0)
        for (int k = 0; k < 3; ++k)
            if ((!(hp.object_dims[k] > 0.f) && !(hp.object_shape == 1 && k == 2)) || !(hp.object_inertia[k] > 0.f))
                return "mi_engine_create: hand task egg / pen need positive object_dims / object_inertia";
    if (!(hp.cube_mass > 0.f)) return "mi_engine_create: hand task object mass must be positive";
    for (int k = 0; hp.obs_type != 0 && k < hp.num_obs; ++k)
        if (hp.obs_map[k] < 0 || hp.obs_map[k] >= nfull) return "mi_engine_create: hand task obs_map entry out of range";
    return nullptr;
}

// mi_engine_create without the engine object: every check, the parameter copy, the arena layout and the defaults, into `e`.  Nothing is allocated
// that outlives a refusal; `out` is only checked.
inline std::string core_create(EngineCore& e, const char* task, const MiSimParams* sim, const void* task_params, size_t task_params_bytes, int num_envs,
                               int env_id_offset, uint64_t seed, void* arena, size_t arena_bytes, const void* out) {
    const int t = task ? find_task(task) : -1;
    if (t < 0) return std::string("unknown task: ") + (task ? task : "(null)");
    if (!sim || !task_params || !arena || !out) return "mi_engine_create: null argument";
    if (num_envs <= 0) return "mi_engine_create: num_envs must be positive";
    if (task_params_bytes != kTasks[t].pbytes) return "mi_engine_create: task_params size mismatch (ABI)";
    if (sim->substeps < 1 || sim->dt <= 0.f) return "mi_engine_create: invalid sim params";
    e = EngineCore{};
    e.task = t; e.N = num_envs; e.steps = 0; e.control_freq_inv = 1; e.clip_obs = INFINITY;
    memcpy(&e.P, sim, sizeof(SimParams));
    e.terrain.walls = 1;
    e.max_init_level = 0;
    if (t == T_CARTPOLE) memcpy(&e.cart, task_params, sizeof(CartpoleParams));
    else if (t == T_ANYMAL) memcpy(&e.anymal, task_params, sizeof(AnymalParams));
    else if (t == T_ANYMAL_FLAT) memcpy(&e.anymal_flat, task_params, sizeof(AnymalFlatParams));
    else if (t == T_QUADCOPTER) memcpy(&e.quad, task_params, sizeof(QuadcopterParams));
    else if (t == T_INGENUITY) {
        memcpy(&e.ing, task_params, sizeof(IngenuityParams));
        if (e.ing.target_period < 1) return "mi_engine_create: Ingenuity target_period must be positive";
    } else if (t == T_BALLBALANCE) {
        memcpy(&e.bbot, task_params, sizeof(BallBalanceParams));
        const BallBalanceParams& b = e.bbot;
        if (!(b.ball_mass > 0.f) || !(b.ball_inertia > 0.f) || !(b.ball_radius > 0.f) || !(b.pin_stiffness >= 0.f) || !(b.pin_damping >= 0.f) ||
            !(b.pin_stiffness + b.pin_damping > 0.f))
            return "mi_engine_create: BallBalance needs positive ball mass / inertia / radius and a non-zero attractor";
    } else if (is_hand_task(t)) {
        memcpy(&e.hand, task_params, sizeof(HandParams));
        if (const char* err = core_check_hand(t, e.hand)) return err;
    } else if (t == T_ARTICULATION) {
        memcpy(&e.artic, task_params, sizeof(ArticulationParams));
        if (!scene_shapes_known(e.artic.scene.n_free, e.artic.scene.free_shape))
            return "mi_engine_create: MiScene.free_shape holds an unknown shape code (0 box, 1 sphere, 2 capsule)";
        core_default_statics(e);
    } else memcpy(&e.loco, task_params, sizeof(LocoParams));
    Layout L;
    build_layout(t, num_envs, L, &e.v, (char*)arena, is_hand_task(t) ? e.hand.num_obs : 0);
    e.lamp_arena = e.v.lamp;       // self-collision is on by default where the reference's actor collides with itself
    e.dof_api_arena = e.v.dof_api; // (AnymalTerrain: the task's lagging dof-state tensor is on by default, as in the reference)
    e.actor_scale_arena = e.v.actor_scale; e.limit_shift_arena = e.v.limit_shift;
    e.v.actor_scale = nullptr; e.v.limit_shift = nullptr;
    memset(&e.hv, 0, sizeof(e.hv));
    e.hv.drive_clamp = 1;
    // the asset's hand-to-hand contact pairs (Shadow Hand, shared.xml:31-51) are on by default; the Allegro hand's URDF lists none
    e.hv.pair_k = (t == T_SHADOWHAND) ? 2.0e4f : 0.f;
    e.hv.tips_in_post = 1;
    e.hv.pre_parts = 4;
    core_task_layout(t, num_envs, L, &e, (char*)arena);
    if (arena_bytes < L.off) return "mi_engine_create: arena too small";
    e.descs = L.d;
    e.v.N = num_envs; e.v.env_offset = env_id_offset; e.v.seed = (uint32_t)(seed ^ (seed >> 32));
    e.v.clip_obs = INFINITY;
    return {};
}

inline std::string core_tensor_desc(const EngineCore* e, int i, MiTensorDesc* out) {
    if (!e || !out || i < 0 || i >= (int)e->descs.size()) return "mi_engine_tensor_desc: bad index";
    *out = e->descs[i];
    return {};
}

// ------------------------------------------------------------------------------------------------ options
// optional knobs of mi_engine_set_option / mi_engine_get_option: one entry per key.  A backend lists the keys only it has (or that it answers
// in its own way) in a table of its own, which is searched first.
enum : unsigned { MI_ON_HIP = 1u, MI_ON_CPU = 2u, MI_ON_BOTH = 3u };
struct EngineOption {
    const char* name;
    unsigned backends;
    std::string (*set)(EngineCore& e, double x);
    double (*get)(const EngineCore& e);
};
#define MI_SET [](EngineCore& e, double x) -> std::string
#define MI_GET [](const EngineCore& e) -> double
// dof_state_lag (AnymalTerrain): PD law / observations / reward read the dof state of the task's last refresh (1, default, the reference's
// behaviour: anymal_terrain.py:441-455 + vec_task.py:379-382) or the physics state (0).  Switching it back on re-synchronises the tensor, which
// is the backend's part: `resync` copies 2 * nd * N floats from v.dof to dof_api_arena (a synchronous copy: this is a set-up call).
template <class Resync>
inline std::string core_set_dof_state_lag(EngineCore& e, double x, Resync resync) {
    if (e.task != T_ANYMAL) return "dof_state_lag: an AnymalTerrain option";
    if (x != 0 && e.v.dof_api == nullptr)
        if (std::string err = resync((size_t)2 * kTasks[e.task].nd * e.N * sizeof(float)); !err.empty()) return err;
    e.v.dof_api = x != 0 ? e.dof_api_arena : nullptr;
    return {};
}
inline double core_get_dof_state_lag(const EngineCore& e) { return (e.task == T_ANYMAL && e.v.dof_api != nullptr) ? 1 : 0; }
static const EngineOption kCoreOptions[] = {
    // env.clipObservations (vec_task.py:115)
    {"clip_obs", MI_ON_BOTH, MI_SET { e.clip_obs = (float)x; e.v.clip_obs = (float)x; return {}; }, MI_GET { return e.clip_obs; }},
    // sim_params.gravity randomisation (reference vec_task.py:720-732 -> gym.set_sim_params)
    {"gravity_x", MI_ON_BOTH, MI_SET { e.P.g[0] = (float)x; return {}; }, MI_GET { return e.P.g[0]; }},
    {"gravity_y", MI_ON_BOTH, MI_SET { e.P.g[1] = (float)x; return {}; }, MI_GET { return e.P.g[1]; }},
    {"gravity_z", MI_ON_BOTH, MI_SET { e.P.g[2] = (float)x; return {}; }, MI_GET { return e.P.g[2]; }},
    // env.controlFrequencyInv (vec_task.py:111)
    {"control_freq_inv", MI_ON_BOTH, MI_SET { if (x < 1) return "control_freq_inv < 1"; e.control_freq_inv = (int)x; return {}; },
     MI_GET { return e.control_freq_inv; }},
    // self-collision of the actor (reference: the collision filter passed to gym.create_actor, humanoid.py:194 uses 0 = collide);
    // only tasks whose arena has the self_contact_impulse tensor accept 1
    {"self_collision", MI_ON_BOTH, MI_SET {
         if (x != 0 && !e.lamp_arena) return "self_collision: this task's actor has no self-collision tables";
         e.v.lamp = x != 0 ? e.lamp_arena : nullptr; return {}; },
     MI_GET { return e.v.lamp != nullptr ? 1.0 : 0.0; }},
    // hands: lanes per env of the pre kernel, 4 (default) or 1
    {"pre_parts", MI_ON_HIP, MI_SET {
         if (!is_hand_task(e.task)) return "pre_parts: a hand-task option";
         if (x != 1 && x != 4) return "pre_parts: 1 or 4";
         e.hv.pre_parts = (int)x; return {}; },
     MI_GET { return is_hand_task(e.task) ? e.hv.pre_parts : 0; }},
    // hands: fingertip states by the post kernel's fingertip groups (1, default) or by hand_tips_kernel (0)
    {"tips_in_post", MI_ON_HIP, MI_SET {
         if (!is_hand_task(e.task)) return "tips_in_post: a hand-task option";
         e.hv.tips_in_post = x != 0 ? 1 : 0; return {}; },
     MI_GET { return is_hand_task(e.task) ? e.hv.tips_in_post : 0; }},
    // ShadowHand: the sub-step reads the per-body link-mass factors of `hand_body_mass_scale` (0, default: it does not)
    {"hand_body_mass", MI_ON_BOTH, MI_SET {
         if (e.task != T_SHADOWHAND) return "hand_body_mass: a ShadowHand option (the Allegro hand's kernels take one mass factor per env)";
         e.hv.body_mass = x != 0 ? e.hv.body_mass_arena : nullptr; return {}; },
     MI_GET { return (is_hand_task(e.task) && e.hv.body_mass != nullptr) ? 1 : 0; }},
    // hands: N/m of the compliant hand-to-hand contact pairs; 0 = the pairs off
    {"hand_pair_stiffness", MI_ON_BOTH, MI_SET {
         if (!is_hand_task(e.task)) return "hand_pair_stiffness: a hand-task option";
         if (!(x >= 0)) return "hand_pair_stiffness: >= 0";
         e.hv.pair_k = (float)x; return {}; },
     MI_GET { return is_hand_task(e.task) ? e.hv.pair_k : 0; }},
    // hands: the position drives deliver at most their force range (shared.xml:250-269, allegro_hand.py:264); default 1
    {"drive_force_limit", MI_ON_BOTH, MI_SET {
         if (!is_hand_task(e.task)) return "drive_force_limit: a hand-task option";
         e.hv.drive_clamp = x != 0 ? 1 : 0; return {}; },
     MI_GET { return is_hand_task(e.task) ? e.hv.drive_clamp : 0; }},
    // limb-per-wave locomotion (Ant): 1 = post_physics_step runs on one wave of every sub-step workgroup at the end of the step's last
    // sub-step launch (mw_kernels.hpp), 0 (default) = in loco_post_kernel as for the one-wave form
    {"fused_post", MI_ON_HIP, MI_SET { e.v.fused_post = x != 0 ? 1 : 0; return {}; }, MI_GET { return e.v.fused_post; }},
    // limb-per-wave sub-steps (Ant, ANYmal on the terrain): all sub-steps of a control step in one launch (View::fused_sub)
    {"fused_sub", MI_ON_HIP, MI_SET { e.v.fused_sub = x != 0 ? 1 : 0; return {}; }, MI_GET { return e.v.fused_sub; }},
    // control-step counter (observation ring parity, AnymalTerrain push schedule, noise counters): part of a state checkpoint
    {"steps", MI_ON_BOTH, MI_SET { if (x < 0) return "steps < 0"; e.steps = (unsigned long long)x; return {}; }, MI_GET { return (double)e.steps; }},
    // 1: the sub-step reads actor_scale / dof_limit_shift (Ant, Humanoid); the hands always read their own factor tensors
    {"actor_tensors", MI_ON_BOTH, MI_SET {
         if (is_hand_task(e.task)) return {};
         if (x != 0 && e.actor_scale_arena == nullptr) return "actor_tensors: this task carries no actor_scale / dof_limit_shift tensors";
         e.v.actor_scale = x != 0 ? e.actor_scale_arena : nullptr;
         e.v.limit_shift = x != 0 ? e.limit_shift_arena : nullptr; return {}; },
     MI_GET { return (is_hand_task(e.task) || e.v.actor_scale != nullptr) ? 1.0 : 0.0; }},
    // static boxes the scene of this library's Articulation unit holds: 4, or 12 for a variant built wide (read-only)
    {"scene_static_capacity", MI_ON_BOTH, MI_SET { (void)e; (void)x; return "scene_static_capacity: read-only (a build property of the library)"; },
     MI_GET { return e.task == T_ARTICULATION ? core_scene_static_capacity() : 0; }},
    // terrain.slopeTreshold of the mesh generator (anymal_terrain.py:576); 0 = off
    {"terrain_slope_threshold", MI_ON_BOTH, MI_SET {
         if (e.task != T_ANYMAL) return "terrain_slope_threshold: only AnymalTerrain has a terrain";
         e.terrain.slope_threshold = (float)x; return {}; },
     MI_GET { return e.terrain.slope_threshold; }},
    // the vertical faces of the slope-corrected triangle mesh (anymal_terrain.py:198-211, :576) collide from the side
    {"terrain_walls", MI_ON_BOTH, MI_SET {
         if (e.task != T_ANYMAL) return "terrain_walls: only AnymalTerrain has a terrain";
         e.terrain.walls = x != 0 ? 1 : 0; return {}; },
     MI_GET { return e.terrain.walls; }},
};

template <size_t NOWN>
inline const EngineOption* core_find_option(const char* key, unsigned backend, const EngineOption (&own)[NOWN]) {
    for (const EngineOption& o : own) if (!strcmp(key, o.name)) return &o;
    for (const EngineOption& o : kCoreOptions) if ((o.backends & backend) && !strcmp(key, o.name)) return &o;
    return nullptr;
}
template <size_t NOWN>
inline std::string core_set_option(EngineCore* e, const char* key, double value, unsigned backend, const EngineOption (&own)[NOWN]) {
    if (!e) return "null engine";
    const EngineOption* o = core_find_option(key, backend, own);
    return o ? o->set(*e, value) : std::string("unknown option: ") + key;
}
template <size_t NOWN>
inline std::string core_get_option(const EngineCore* e, const char* key, double* out, unsigned backend, const EngineOption (&own)[NOWN]) {
    if (!e || !key || !out) return "mi_engine_get_option: null argument";
    const EngineOption* o = core_find_option(key, backend, own);
    if (!o) return std::string("unknown option: ") + key;
    *out = o->get(*e);
    return {};
}

inline std::string core_set_noise(EngineCore* e, int which, const MiNoiseParams* p) {
    if (!e || !p) return "mi_engine_set_noise: null argument";
    if (which != 0 && which != 1) return "mi_engine_set_noise: which must be 0 (observations) or 1 (actions)";
    if (p->dist < 0 || p->dist > 2 || p->op < 0 || p->op > 1) return "mi_engine_set_noise: dist in {0,1,2}, op in {0,1}";
    if (e->task != T_CARTPOLE && e->task != T_ANT && e->task != T_HUMANOID && !is_hand_task(e->task) && p->dist != 0)
        return "mi_engine_set_noise: in-kernel noise exists for Cartpole, Ant, Humanoid and ShadowHand";
    memcpy(which == 0 ? &e->v.obs_noise : &e->v.act_noise, p, sizeof(NoiseParams));
    return {};
}
inline int core_last_ring(const EngineCore* e) { return e ? (int)((e->steps + 1) & 1) : -1; }

inline std::string core_check_terrain_args(const EngineCore* e, const int16_t* height_samples, int rows, int cols, float horizontal_scale,
                                           const float* env_origins, int num_levels, int num_terrains) {
    if (!e) return "null engine";
    if (e->task != T_ANYMAL) return "mi_engine_set_terrain: only AnymalTerrain uses a terrain";
    if (!height_samples || !env_origins || rows < 2 || cols < 2 || num_levels < 1 || num_terrains < 1 || horizontal_scale <= 0.f)
        return "mi_engine_set_terrain: bad argument";
    return {};
}
// hs / origins: where the engine reads the (checked) arrays from -- the caller's device arrays, or the CPU backend's copies
inline void core_set_terrain(EngineCore& e, const short* hs, int rows, int cols, float horizontal_scale, float vertical_scale, float border_size,
                             const float* origins, int num_levels, int num_terrains, float env_length, int max_init_level) {
    e.terrain.hs = hs; e.terrain.rows = rows; e.terrain.cols = cols;
    e.terrain.hscale = horizontal_scale; e.terrain.vscale = vertical_scale; e.terrain.border = border_size;
    e.terrain.origins = origins; e.terrain.levels = num_levels; e.terrain.types = num_terrains;
    e.terrain.env_length = env_length;
    e.max_init_level = max_init_level < 0 ? 0 : (max_init_level >= num_levels ? num_levels - 1 : max_init_level);
}

// ------------------------------------------------------------------------------------------------ initial state
// the view the initial state is written through: the `actor_params` tensors are initialised whether the sub-step reads them or not
inline View init_view(const EngineCore& e) {
    View v = e.v;
    v.actor_scale = e.actor_scale_arena; v.limit_shift = e.limit_shift_arena;
    return v;
}
// height of the root at rest (cartpole.py:93 / ant.py:164 / the tasks' default poses); the hands have an initial state of their own
inline float core_init_root_z(const EngineCore& e) {
    switch (e.task) {
        case T_CARTPOLE: return 2.0f;
        case T_QUADCOPTER: return e.quad.init_height;
        case T_INGENUITY: return e.ing.init_height;
        case T_BALLBALANCE: return e.bbot.tray_height;
        case T_ANYMAL: return e.anymal.base_init_state[2];
        case T_ANYMAL_FLAT: return e.anymal_flat.base_init_state[2];
        case T_ARTICULATION: return e.artic.init_root[2];
        default: return e.loco.start_height;
    }
}
inline bool core_is_loco(const EngineCore& e) { return e.task == T_ANT || e.task == T_HUMANOID; }
inline float core_init_potential(const EngineCore& e) { return core_is_loco(e) ? -1000.f / e.loco.dt : 0.f; }      // ant.py:113
// the constants of env e of a fresh engine (v: init_view); init_dof: [nd] start joint positions, or null for zeros
MI_HD void init_env_constants(const View& v, int e, int nd, int nsph3, int nsens6, int nobs, int nact, float root_z, const float* init_dof, float pot0) {
    const int N = v.N;
    const float root[13] = {0, 0, root_z, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 13; ++k) { v.root[k * N + e] = root[k]; v.init_root[k * N + e] = root[k]; }
    for (int k = 0; k < nd; ++k) {
        v.dof[k * N + e] = init_dof ? init_dof[k] : 0.f;
        v.dof[(nd + k) * N + e] = 0.f;
        v.tau[k * N + e] = 0.f; v.laml[k * N + e] = 0.f; v.dof_force[k * N + e] = 0.f;
    }
    for (int k = 0; k < nsph3; ++k) v.lamc[k * N + e] = 0.f;
    if (v.lamp) for (int k = 0; k < 3 * ModelHumanoid::NPG; ++k) { v.lamp[k * N + e] = 0.f; v.pairf[k * N + e] = 0.f; }
    if (v.dropped) { v.dropped[e] = 0; v.dropped[N + e] = 0; }
    for (int k = 0; k < nsens6; ++k) v.sensor[k * N + e] = 0.f;
    for (int k = 0; k < nact; ++k) v.actions[k * N + e] = 0.f;
    for (int k = 0; k < nobs; ++k) { v.obs[(size_t)e * nobs + k] = 0.f; v.obs_out[(size_t)e * nobs + k] = 0.f; v.obs_out[((size_t)N + e) * nobs + k] = 0.f; }
    v.potentials[e] = pot0; v.prev_potentials[e] = pot0;
    if (v.friction) v.friction[e] = -1.f;       // model friction until somebody writes the tensor (AnymalTerrain's init overwrites it)
    if (v.actor_scale) for (int k = 0; k < v.nas; ++k) v.actor_scale[k * N + e] = 1.f;
    if (v.limit_shift) for (int k = 0; k < 2 * nd; ++k) v.limit_shift[k * N + e] = 0.f;
    for (int k = 0; k < 3; ++k) { v.up_vec[k * N + e] = (k == 2) ? 1.f : 0.f; v.heading_vec[k * N + e] = (k == 0) ? 1.f : 0.f; }
    v.rew[e] = 0.f;
    v.reset[e] = 1;  // vec_task.py:316-317: every env is reset inside the first step()
    v.progress[e] = 0; v.randomize[e] = 0; v.timeout[e] = 0; v.episode[e] = 0;
    v.ep_ret[e] = 0.f;
    if (e == 0) for (int k = 0; k < 8; ++k) v.stats[k] = 0.f;
}
