// lifecycle_host.cpp -- csrc/engine_core.hpp behind a trivial backend, on a malloc'ed arena: the create / option / noise / terrain part of the
// transcript of tests/test_lifecycle_twins.py, every refused input included, and the initial-state constants of every env written through the
// arena of exactly core_arena_bytes().  A program of its own so that it can be built with -fsanitize=address,undefined and run as it is:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/hostbuild/lifecycle_host.cpp -o lifecycle_host && ./lifecycle_host
// Exit status 0 and "lifecycle_host ok" when every call answered as expected.
#include <cstdio>
#include <cstdlib>

#include "../../isaacgymenvs_amd/csrc/engine_core.hpp"
#include "../../isaacgymenvs_amd/csrc/gen/model_articulation.h"

ArticulationMeta mi_articulation_meta() {
    using AM = ModelArticulation;
    return ArticulationMeta{AM::ND, AM::NB, AM::NSENS, AM::NSPH, AM::FIXED};
}

struct MiEngine : EngineCore { int knob = 0; };
constexpr unsigned BACKEND = MI_ON_CPU;
static const EngineOption kOwnOptions[] = {
    {"knob", BACKEND, MI_SET { if (x < 0) return "knob < 0"; static_cast<MiEngine&>(e).knob = (int)x; return {}; },
     MI_GET { return static_cast<const MiEngine&>(e).knob; }},
};

static int g_failed = 0;
constexpr int N = 70;
static void expect(bool want_ok, const std::string& err, const char* what, const char* task) {
    if (err.empty() != want_ok) { printf("FAILED %s / %s: %s\n", task, what, err.empty() ? "accepted" : err.c_str()); ++g_failed; }
}

union Params {
    MiCartpoleParams cart; MiLocoParams loco; MiAnymalParams anymal; MiAnymalFlatParams flat; MiQuadcopterParams quad; MiIngenuityParams ing;
    MiBallBalanceParams bbot; MiHandParams hand; MiArticulationParams artic;
};
static Params valid_params(int t) {
    Params p;
    memset(&p, 0, sizeof(p));
    if (is_hand_task(t)) { p.hand.obs_type = 0; p.hand.num_obs = kTasks[t].nobs; p.hand.cube_mass = 0.07f; }
    if (t == T_INGENUITY) p.ing.target_period = 500;
    if (t == T_BALLBALANCE) { p.bbot.ball_mass = 0.84f; p.bbot.ball_inertia = 3.4e-3f; p.bbot.ball_radius = 0.1f; p.bbot.pin_stiffness = 5e7f; }
    return p;
}

int main() {
    MiSimParams sim;
    memset(&sim, 0, sizeof(sim));
    sim.dt = 0.0166f; sim.substeps = 2; sim.iters = 4;
    MiTaskInfo info;
    expect(false, core_task_info("Nope", &info), "task_info unknown", "-");
    expect(false, core_task_info(nullptr, &info), "task_info null task", "-");
    expect(false, core_task_info("Ant", nullptr), "task_info null out", "-");
    if (core_arena_bytes("Nope", 8) != 0 || core_arena_bytes("Ant", 0) != 0 || core_arena_bytes(nullptr, 8) != 0) { printf("FAILED arena_bytes of a bad request\n"); ++g_failed; }
    for (int t = 0; t < kNumTasks; ++t) {
        const char* task = kTasks[t].name;
        expect(true, core_task_info(task, &info), "task_info", task);
        const size_t nbytes = core_arena_bytes(task, N);
        char* arena = (char*)malloc(nbytes);
        MiEngine eng, *out = &eng;
        Params tp = valid_params(t);
        const size_t pb = kTasks[t].pbytes;
        auto create = [&](bool ok, const char* what, const Params& p, const MiSimParams* s = nullptr, int n = N, size_t bytes = 0, size_t abytes = 0, bool nul = false) {
            MiEngine scratch;
            expect(ok, core_create(scratch, task, s ? s : &sim, nul ? nullptr : &p, bytes ? bytes : pb, n, 0, 1, arena, abytes ? abytes : nbytes, &out), what, task);
        };
        create(true, "valid", tp);
        expect(false, core_create(eng, "Nope", &sim, &tp, pb, N, 0, 1, arena, nbytes, &out), "unknown task", task);
        expect(false, core_create(eng, task, nullptr, &tp, pb, N, 0, 1, arena, nbytes, &out), "null sim", task);
        expect(false, core_create(eng, task, &sim, &tp, pb, N, 0, 1, nullptr, nbytes, &out), "null arena", task);
        expect(false, core_create(eng, task, &sim, &tp, pb, N, 0, 1, arena, nbytes, nullptr), "null out", task);
        create(false, "null task_params", tp, nullptr, N, 0, 0, true);
        create(false, "task_params_bytes=12", tp, nullptr, N, 12);
        create(false, "num_envs=0", tp, nullptr, 0);
        create(false, "arena one byte short", tp, nullptr, N, 0, nbytes - 1);
        MiSimParams bad = sim;
        bad.dt = 0.f;
        create(false, "dt=0", tp, &bad);
        bad = sim; bad.substeps = 0;
        create(false, "substeps=0", tp, &bad);
        if (is_hand_task(t)) {
            Params p = tp; p.hand.obs_type = 5; create(false, "obs_type=5", p);
            p = tp; p.hand.num_obs = 10; create(false, "num_obs=10", p);
            p = tp; p.hand.obs_type = 1; p.hand.num_obs = 500; create(false, "num_obs=500", p);
            p = tp; p.hand.object_shape = 3; create(false, "object_shape=3", p);
            p = tp; p.hand.object_shape = 2; create(false, "egg no dims", p);
            p.hand.object_dims[0] = p.hand.object_dims[1] = 0.03f; p.hand.object_dims[2] = 0.04f; create(false, "egg no inertia", p);
            p.hand.object_inertia[0] = p.hand.object_inertia[1] = 7.5e-5f; p.hand.object_inertia[2] = 5.4e-5f; create(true, "egg", p);
            p.hand.object_shape = 1; p.hand.object_dims[2] = 0.f; create(true, "pen", p);
            p = tp; p.hand.cube_mass = 0.f; create(false, "cube_mass=0", p);
            p = tp; p.hand.obs_type = 1; p.hand.num_obs = 4; create(true, "obs_type=1", p);
            p.hand.obs_map[2] = (short)kTasks[t].nobs; create(false, "obs_map[2]=nfull", p);
            p.hand.obs_map[2] = -1; create(false, "obs_map[2]=-1", p);
        }
        if (t == T_INGENUITY) { Params p = tp; p.ing.target_period = 0; create(false, "target_period=0", p); }
        if (t == T_BALLBALANCE) {
            Params p = tp; p.bbot.ball_mass = 0.f; create(false, "ball_mass=0", p);
            p = tp; p.bbot.ball_radius = 0.f; create(false, "ball_radius=0", p);
            p = tp; p.bbot.ball_inertia = 0.f; create(false, "ball_inertia=0", p);
            p = tp; p.bbot.pin_stiffness = 0.f; create(false, "no attractor", p);
            p = tp; p.bbot.pin_stiffness = -1.f; p.bbot.pin_damping = 5.f; create(false, "pin_stiffness<0", p);
            p = tp; p.bbot.pin_damping = -1.f; create(false, "pin_damping<0", p);
        }
        if (t == T_ARTICULATION) {
            Params p = tp; p.artic.scene.n_free = 2; p.artic.scene.free_shape = 0x30; create(false, "free_shape code 3", p);
            p.artic.scene.free_shape = 0x21; create(true, "free_shape sphere capsule", p);
        }
        expect(true, core_create(eng, task, &sim, &tp, pb, N, 0, 1, arena, nbytes, &out), "create", task);

        // every tensor, then the initial-state constants of every env, through the arena of exactly nbytes
        MiTensorDesc d;
        for (int i = 0; i < (int)eng.descs.size(); ++i) expect(true, core_tensor_desc(&eng, i, &d), "tensor_desc", task);
        expect(false, core_tensor_desc(&eng, (int)eng.descs.size(), &d), "tensor_desc index n", task);
        expect(false, core_tensor_desc(&eng, -1, &d), "tensor_desc index -1", task);
        expect(false, core_tensor_desc(&eng, 0, nullptr), "tensor_desc null out", task);
        if (!is_hand_task(t)) {
            const TaskMeta& m = kTasks[t];
            const View v = init_view(eng);
            for (int en = 0; en < N; ++en)
                init_env_constants(v, en, m.nd, 3 * m.nsph, 6 * m.nsens, m.nobs, m.nact, core_init_root_z(eng), core_is_loco(eng) ? eng.loco.initial_dof_pos : nullptr,
                                   core_init_potential(eng));
            if (v.reset[N - 1] != 1 || v.root[6 * N + N - 1] != 1.f) { printf("FAILED %s: initial state\n", task); ++g_failed; }
        }

        const bool hand = is_hand_task(t), terr = t == T_ANYMAL, tensors = t == T_ANT || t == T_HUMANOID || t == T_ANYMAL_FLAT;
        struct { const char* key; double x; bool ok; } sets[] = {
            {"clip_obs", 5.0, true}, {"gravity_x", -3.5, true}, {"gravity_y", 0.25, true}, {"gravity_z", -1.5, true}, {"control_freq_inv", 2.0, true},
            {"control_freq_inv", 0.0, false}, {"self_collision", 0.0, true}, {"self_collision", 1.0, t == T_HUMANOID}, {"hand_body_mass", 1.0, t == T_SHADOWHAND},
            {"hand_pair_stiffness", 100.0, hand}, {"hand_pair_stiffness", -1.0, false}, {"hand_pair_stiffness", NAN, false}, {"drive_force_limit", 0.0, hand},
            {"steps", 7.0, true}, {"steps", -1.0, false}, {"actor_tensors", 1.0, hand || tensors}, {"actor_tensors", 0.0, true},
            {"terrain_slope_threshold", 0.75, terr}, {"terrain_walls", 0.0, terr}, {"knob", 3.0, true}, {"knob", -3.0, false},
            // keys of the other backend, and of none
            {"pre_parts", 1.0, false}, {"tips_in_post", 0.0, false}, {"fused_post", 1.0, false}, {"fused_sub", 1.0, false}, {"no_such_option", 1.0, false}};
        for (const auto& s : sets) {
            expect(s.ok, core_set_option(&eng, s.key, s.x, BACKEND, kOwnOptions), s.key, task);
            double got = -1;
            const bool known = core_find_option(s.key, BACKEND, kOwnOptions) != nullptr;
            expect(known, core_get_option(&eng, s.key, &got, BACKEND, kOwnOptions), s.key, task);
        }
        double got = -1;
        expect(true, core_get_option(&eng, "pre_parts", &got, MI_ON_HIP, kOwnOptions), "pre_parts on the other backend", task);
        expect(false, core_set_option(nullptr, "steps", 1.0, BACKEND, kOwnOptions), "set_option null engine", task);
        expect(false, core_get_option(nullptr, "steps", &got, BACKEND, kOwnOptions), "get_option null engine", task);
        expect(false, core_get_option(&eng, nullptr, &got, BACKEND, kOwnOptions), "get_option null key", task);
        expect(false, core_get_option(&eng, "steps", nullptr, BACKEND, kOwnOptions), "get_option null out", task);
        if (eng.knob != 3 || core_last_ring(&eng) != 0 || core_last_ring(nullptr) != -1) { printf("FAILED %s: knob / last_ring\n", task); ++g_failed; }

        const bool noisy = t == T_CARTPOLE || t == T_ANT || t == T_HUMANOID || hand;
        MiNoiseParams np;
        memset(&np, 0, sizeof(np));
        expect(true, core_set_noise(&eng, 0, &np), "noise off", task);
        np.dist = 1; expect(noisy, core_set_noise(&eng, 0, &np), "noise gaussian", task);
        expect(false, core_set_noise(&eng, 2, &np), "noise which=2", task);
        expect(false, core_set_noise(&eng, -1, &np), "noise which=-1", task);
        np.dist = 3; expect(false, core_set_noise(&eng, 0, &np), "noise dist=3", task);
        np.dist = -1; expect(false, core_set_noise(&eng, 0, &np), "noise dist=-1", task);
        np.dist = 1; np.op = 2; expect(false, core_set_noise(&eng, 1, &np), "noise op=2", task);
        np.op = -1; expect(false, core_set_noise(&eng, 1, &np), "noise op=-1", task);
        expect(false, core_set_noise(&eng, 0, nullptr), "noise null params", task);
        expect(false, core_set_noise(nullptr, 0, &np), "noise null engine", task);

        int16_t hs[4 * 5] = {0};
        float origins[2 * 3 * 3] = {0};
        expect(terr, core_check_terrain_args(&eng, hs, 4, 5, 0.1f, origins, 2, 3), "terrain", task);
        expect(false, core_check_terrain_args(nullptr, hs, 4, 5, 0.1f, origins, 2, 3), "terrain null engine", task);
        expect(false, core_check_terrain_args(&eng, nullptr, 4, 5, 0.1f, origins, 2, 3), "terrain null height_samples", task);
        expect(false, core_check_terrain_args(&eng, hs, 4, 5, 0.1f, nullptr, 2, 3), "terrain null env_origins", task);
        expect(false, core_check_terrain_args(&eng, hs, 1, 5, 0.1f, origins, 2, 3), "terrain rows=1", task);
        expect(false, core_check_terrain_args(&eng, hs, 4, 1, 0.1f, origins, 2, 3), "terrain cols=1", task);
        expect(false, core_check_terrain_args(&eng, hs, 4, 5, 0.1f, origins, 0, 3), "terrain num_levels=0", task);
        expect(false, core_check_terrain_args(&eng, hs, 4, 5, 0.1f, origins, 2, 0), "terrain num_terrains=0", task);
        expect(false, core_check_terrain_args(&eng, hs, 4, 5, 0.f, origins, 2, 3), "terrain horizontal_scale=0", task);
        if (terr) {
            for (int lvl : {-2, 1, 9}) {
                core_set_terrain(eng, hs, 4, 5, 0.1f, 0.005f, 0.5f, origins, 2, 3, 8.f, lvl);
                if (eng.max_init_level != (lvl < 0 ? 0 : lvl > 1 ? 1 : lvl)) { printf("FAILED max_init_level clamp of %d\n", lvl); ++g_failed; }
            }
        }
        free(arena);
    }
    if (g_failed) { printf("lifecycle_host: %d check(s) failed\n", g_failed); return 1; }
    printf("lifecycle_host ok\n");
    return 0;
}
