// quadcopter_step.hpp -- the Quadcopter control step for ONE env around gym.simulate(), host + device: what kernels_quadcopter.hip runs per
// lane and cpu/mi_engine_cpu.cpp per loop iteration (reference isaacgymenvs/tasks/quadcopter.py).  Reduction policy: tasks/loco_step.hpp.
#pragma once
#include "../task_views.hpp"
#include "loco_step.hpp"
#include "quadcopter.hpp"

namespace mi {

// reset_idx (:254-274), deferred (from pre_physics_step) or indexed: the draws of the env's current episode number.  q: [kQuadDof] out, the
// joint positions it stored (the pre step makes them the targets; handed back so that it does not read them from memory again)
MI_HD void quad_reset_env(const View& v, const QuadView&, const QuadcopterParams& p, const int e, float* q) {
    const int N = v.N;
    float root[13], qd[kQuadDof];
    const int ep = v.episode[e];
    quadcopter_reset(p, v.seed, (uint32_t)(v.env_offset + e), (uint32_t)ep, root, q, qd);
    for (int k = 0; k < 13; ++k) v.root[k * N + e] = root[k];
    for (int d = 0; d < kQuadDof; ++d) { v.dof[d * N + e] = q[d]; v.dof[(kQuadDof + d) * N + e] = 0.f; v.laml[d * N + e] = 0.f; }
    v.episode[e] = ep + 1;
    v.reset[e] = 0;       // :273-274
    v.progress[e] = 0;
}

// pre_physics_step (:276-292)
MI_HD void quad_pre_env(const View& v, const QuadView& qv, const QuadcopterParams& p, const float* __restrict__ actions_in, const int e) {
    MI_NO_CONTRACT
    const int N = v.N;
    const bool rs = v.reset[e] != 0;
    float q[kQuadDof];
    if (rs) quad_reset_env(v, qv, p, e, q);                                                                   // reset_idx(reset_env_ids) (:279-281)
    for (int d = 0; d < kQuadDof; ++d) {
        const float a = fminf(fmaxf(actions_in[(size_t)e * kQuadAct + d], -p.clip_actions), p.clip_actions);   // vec_task.py:374
        v.actions[d * N + e] = a;
        float t = qv.targets[d * N + e] + p.dt * p.dof_action_speed_scale * a;                                 // :284
        t = fmaxf(fminf(t, p.dof_upper[d]), p.dof_lower[d]);                                                   // tensor_clamp (:285)
        if (rs) t = q[d];                                                                                      // :297
        qv.targets[d * N + e] = t;
    }
    for (int k = 0; k < kQuadRotors; ++k) {
        const float a = fminf(fmaxf(actions_in[(size_t)e * kQuadAct + kQuadDof + k], -p.clip_actions), p.clip_actions);
        v.actions[(kQuadDof + k) * N + e] = a;
        float th = qv.thrusts[k * N + e] + p.dt * p.thrust_action_speed_scale * a;                             // :288
        th = fmaxf(fminf(th, p.max_thrust), 0.f);                                                              // :289
        // the reference fills `forces` from the thrusts BEFORE it clears both for the reset envs (:291-296)
        qv.thrusts[k * N + e] = rs ? 0.f : th;
        qv.forces[(3 * ModelQuadcopter::sens_body[k] + 2) * N + e] = rs ? 0.f : th;
    }
}

// post_physics_step (:294-302): progress++, observations, reward
template <class RED>
MI_HD void quad_post_env(const View& v, const QuadView&, const QuadcopterParams& p, const int e0, const RED& red) {
    const int N = v.N;
    const bool valid = e0 < N;
    const int e = valid ? e0 : N - 1;
    float root[13], q[kQuadDof];
    sfor<13>([&](auto K) MI_LAMBDA { root[K] = v.root[K * N + e]; });
    sfor<kQuadDof>([&](auto K) MI_LAMBDA { q[K] = v.dof[K * N + e]; });
    const long long progress = v.progress[e] + 1;
    float obs[kQuadObs], rew;
    long long reset;
    quadcopter_observations(root, q, obs);
    quadcopter_reward(root, progress, p.max_episode_length, &rew, &reset);
    red.episode(v, e, valid, rew, reset, progress);
    if (valid) store_step_outputs(v, e, obs, rew, reset, progress, p.max_episode_length);
}

// the task's own tensors of the __init__ state (:62-101): zero targets / thrusts / forces (the craft's pose: engine_core.hpp init_env_constants)
MI_HD void quad_init_env(const View& v, const QuadView& qv, const QuadcopterParams&, const int e) {
    const int N = v.N;
    for (int d = 0; d < kQuadDof; ++d) qv.targets[d * N + e] = 0.f;
    for (int k = 0; k < kQuadRotors; ++k) qv.thrusts[k * N + e] = 0.f;
    for (int k = 0; k < 3 * ModelQuadcopter::NB; ++k) qv.forces[k * N + e] = 0.f;
}

}  // namespace mi
