// cpu_engine.hpp -- what the translation units of the CPU backend share: the engine object (the lifecycle core of csrc/engine_core.hpp plus what
// only this backend has), the per-thread statistics accumulators and the host's reduction policy for them.
// (cpu/mi_engine_cpu.cpp: C ABI + Cartpole / Ant / Humanoid / Quadcopter / Ingenuity / BallBalance; cpu/cpu_anymal.cpp: AnymalTerrain, Anymal;
//  cpu/cpu_articulation.cpp: the run-time robot; cpu/cpu_hand.cpp, compiled once per hand and object shape: ShadowHand, AllegroHand.)
#pragma once
#include <omp.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../core/engine.hpp"
#include "../engine_core.hpp"

using namespace mi;

struct MiEngine : EngineCore {
    int num_threads;                    // sim.physx.num_threads: OpenMP threads over envs
    std::vector<short> terrain_hs;      // mi_engine_set_terrain copies the caller's arrays: `terrain` points into these two
    std::vector<float> terrain_origins;
};

// job statistics (View::stats) of one OpenMP thread; added up in thread order after the loop over envs
struct StatAcc { double fin_ret = 0, fin_len = 0, fin = 0, r = 0, cnt = 0; };
static inline void episode_stats_env(const View& v, int en, float rew, long long reset, long long progress, StatAcc& a) {
    float ret = v.ep_ret[en] + rew;
    a.r += rew; a.cnt += 1;
    if (reset != 0) { a.fin_ret += ret; a.fin_len += (double)(progress + 1); a.fin += 1; ret = 0.f; }
    v.ep_ret[en] = ret;
}
// the job-statistics reduction policy of the per-env post bodies shared with the kernels (tasks/*_step.hpp); the host has no shadow lanes
struct HostEpisodeRed {
    StatAcc* st;
    void episode(const View& v, int e, bool valid, float rew, long long reset, long long progress) const {
        if (valid) episode_stats_env(v, e, rew, reset, progress, *st);
    }
};
static inline void flush_stats(const View& v, const std::vector<StatAcc>& accs) {
    for (const StatAcc& a : accs) { v.stats[0] += (float)a.fin_ret; v.stats[1] += (float)a.fin_len; v.stats[2] += (float)a.fin; v.stats[3] += (float)a.r; v.stats[4] += (float)a.cnt; }
}

// the tasks of the other translation units: rc 0, or -1 with *err set
int cpu_anymal_init(MiEngine* e, std::string* err);
int cpu_anymal_step(MiEngine* e, const float* actions, bool simulate_only);
int cpu_anymal_reset(MiEngine* e, const int64_t* ids, int n);
int cpu_anymal_body_states(MiEngine* e);
int cpu_anymal_kinematics(MiEngine* e, float* out_j, float* out_h);
int cpu_articulation_reset(MiEngine* e, const int64_t* ids, int n);      // ids == nullptr: every env
int cpu_articulation_simulate(MiEngine* e);
int cpu_articulation_body_states(MiEngine* e);
int cpu_articulation_kinematics(MiEngine* e, float* out_j, float* out_h);
int cpu_hand_init(MiEngine* e);
int cpu_hand_step(MiEngine* e, const float* actions, bool simulate_only);
int cpu_hand_reset(MiEngine* e, const int64_t* ids, int n);
int cpu_hand_body_states(MiEngine* e);
int cpu_hand_kinematics(MiEngine* e, float* out_j, float* out_h);
