// ball_balance_step.hpp -- the BallBalance control step for ONE env around gym.simulate(), host + device: what kernels_ball_balance.hip runs
// per lane and cpu/mi_engine_cpu.cpp per loop iteration (reference isaacgymenvs/tasks/ball_balance.py).  Reduction policy: tasks/loco_step.hpp.
#pragma once
#include "../task_views.hpp"
#include "loco_step.hpp"
#include "ball_balance.hpp"

namespace mi {

// reset_idx (:349-393), deferred (from pre_physics_step) or indexed.  The targets are the caller's: the pre step clears them through its
// `rs ? 0 : t`, the indexed reset by itself.
MI_HD void bbot_reset_env(const View& v, const BbotView& bv, const BallBalanceParams& p, const int e) {
    const int N = v.N;
    const int ep = v.episode[e];
    float ball[13];
    bbot_reset_ball(p, v.seed, (uint32_t)(v.env_offset + e), (uint32_t)ep, ball);
    for (int k = 0; k < 13; ++k) {
        v.root[k * N + e] = v.init_root[k * N + e];                              // :353
        bv.ball[k * N + e] = ball[k];
    }
    for (int d = 0; d < kBbotDof; ++d) { v.dof[d * N + e] = 0.f; v.dof[(kBbotDof + d) * N + e] = 0.f; v.laml[d * N + e] = 0.f; }   // initial_dof_states (:387)
    for (int k = 0; k < 9; ++k) bv.lamp[k * N + e] = 0.f;
    v.episode[e] = ep + 1;
    v.reset[e] = 0;
    v.progress[e] = 0;
}

// pre_physics_step (:395-413)
MI_HD void bbot_pre_env(const View& v, const BbotView& bv, const BallBalanceParams& p, const float* __restrict__ actions_in, const int e) {
    MI_NO_CONTRACT
    const int N = v.N;
    const bool rs = v.reset[e] != 0;
    if (rs) bbot_reset_env(v, bv, p, e);
    float a[kBbotAct];
    for (int k = 0; k < kBbotAct; ++k) {
        a[k] = fminf(fmaxf(actions_in[(size_t)e * kBbotAct + k], -p.clip_actions), p.clip_actions);   // vec_task.py:374
        v.actions[k * N + e] = a[k];
    }
    for (int d = 0; d < kBbotDof; ++d) {
        float t = bv.targets[d * N + e];
        if (d & 1) t += p.dt * p.action_speed_scale * a[d >> 1];                 // actuated dofs 1, 3, 5 (:405)
        t = fmaxf(fminf(t, p.dof_upper[d]), p.dof_lower[d]);                     // tensor_clamp (:406)
        bv.targets[d * N + e] = rs ? 0.f : t;                                    // :409
    }
}

// post_physics_step (:415-424): progress++, observations, reward
template <class RED>
MI_HD void bbot_post_env(const View& v, const BbotView& bv, const BallBalanceParams& p, const int e0, const RED& red) {
    const int N = v.N;
    const bool valid = e0 < N;
    const int e = valid ? e0 : N - 1;
    float q[kBbotDof], qd[kBbotDof], ball[13], sens[6 * kBbotSensors];
    sfor<kBbotDof>([&](auto K) MI_LAMBDA { q[K] = v.dof[K * N + e]; qd[K] = v.dof[(kBbotDof + K) * N + e]; });
    sfor<13>([&](auto K) MI_LAMBDA { ball[K] = bv.ball[K * N + e]; });
    sfor<6 * kBbotSensors>([&](auto K) MI_LAMBDA { sens[K] = v.sensor[K * N + e]; });
    const long long progress = v.progress[e] + 1;
    float obs[kBbotObs], rew;
    long long reset;
    bbot_observations(q, qd, ball, sens, obs);
    bbot_reward(ball, ball + 7, p.ball_radius, v.reset[e], progress, p.max_episode_length, &rew, &reset);
    red.episode(v, e, valid, rew, reset, progress);
    if (valid) store_step_outputs(v, e, obs, rew, reset, progress, p.max_episode_length);
}

// the task's own tensors of the __init__ state (:88-112): ball at its spawn pose, zero targets (the bot's pose: engine_core.hpp init_env_constants)
MI_HD void bbot_init_env(const View& v, const BbotView& bv, const BallBalanceParams& p, const int e) {
    const int N = v.N;
    for (int k = 0; k < 13; ++k) bv.ball[k * N + e] = (k < 3) ? p.ball_init_pos[k] : (k == 6 ? 1.f : 0.f);
    for (int d = 0; d < kBbotDof; ++d) bv.targets[d * N + e] = 0.f;
    for (int k = 0; k < 9; ++k) bv.lamp[k * N + e] = 0.f;
    bv.ncontact[e] = 0;
}

}  // namespace mi
