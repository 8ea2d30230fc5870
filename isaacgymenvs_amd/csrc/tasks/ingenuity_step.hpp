// ingenuity_step.hpp -- the Ingenuity control step for ONE env around gym.simulate(), host + device: what kernels_ingenuity.hip runs per lane
// and cpu/mi_engine_cpu.cpp per loop iteration (reference isaacgymenvs/tasks/ingenuity.py).  Reduction policy: tasks/loco_step.hpp.
#pragma once
#include "../task_views.hpp"
#include "loco_step.hpp"
#include "ingenuity.hpp"

namespace mi {

MI_HD void ing_set_target(const View& v, const IngenuityView& iv, const int e, const float* target) {
    const int N = v.N;
    for (int k = 0; k < 3; ++k) { iv.target[k * N + e] = target[k]; iv.marker[k * N + e] = target[k] + (k == 2 ? 0.4f : 0.f); }   // :288-290
}

// reset_idx (:295-319), deferred (from pre_physics_step) or indexed: the draws of the env's current episode number ep = v.episode[e] (the
// pre step holds it in a register already)
MI_HD void ing_reset_env(const View& v, const IngenuityView& iv, const IngenuityParams& p, const int e, const int ep) {
    const int N = v.N;
    const uint32_t genv = (uint32_t)(v.env_offset + e);
    float root[13], target[3];
    ingenuity_target(v.seed, genv, (uint32_t)ep, 3u, target);
    ing_set_target(v, iv, e, target);
    ingenuity_reset_root(p, v.seed, genv, (uint32_t)ep, root);
    for (int k = 0; k < 13; ++k) v.root[k * N + e] = root[k];
    // set_dof_state_tensor_indexed pushes the tensor as it is: positions unchanged, the two visual rotors' speeds overwritten
    v.dof[(kIngDof + 1) * N + e] = -p.rotor_speed;
    v.dof[(kIngDof + 3) * N + e] = p.rotor_speed;
    for (int d = 0; d < kIngDof; ++d) v.laml[d * N + e] = 0.f;
    v.episode[e] = ep + 1;
    v.reset[e] = 0;       // :316-317
    v.progress[e] = 0;
}

// pre_physics_step (:321-354): the periodic target of the running episode first, then the deferred resets, then the thrusts
MI_HD void ing_pre_env(const View& v, const IngenuityView& iv, const IngenuityParams& p, const float* __restrict__ actions_in, const int e) {
    MI_NO_CONTRACT
    const int N = v.N;
    const int ep = v.episode[e];
    const long long progress = v.progress[e];
    if (progress % p.target_period == 0) {                                          // :324-327
        float target[3];
        ingenuity_target(v.seed, (uint32_t)(v.env_offset + e), (uint32_t)ep, 8u + 3u * (uint32_t)(progress / p.target_period), target);
        ing_set_target(v, iv, e, target);
    }
    const bool rs = v.reset[e] != 0;
    if (rs) ing_reset_env(v, iv, p, e, ep);                                          // reset_idx(reset_env_ids) (:329-332)
    float a[kIngAct];
    for (int k = 0; k < kIngAct; ++k) {
        a[k] = fminf(fmaxf(actions_in[(size_t)e * kIngAct + k], -p.clip_actions), p.clip_actions);   // vec_task.py:374
        v.actions[k * N + e] = a[k];
    }
    for (int r = 0; r < kIngRotors; ++r) {                                          // :337-348
        const float vertical = fminf(fmaxf(a[3 * r + 2] * p.thrust_action_speed_scale, -p.thrust_upper_limit), p.thrust_upper_limit);
        float th[3];
        th[2] = p.dt * vertical;
        for (int k = 0; k < 2; ++k) th[k] = th[2] * fminf(fmaxf(a[3 * r + k], -p.thrust_lateral_component), p.thrust_lateral_component);
        for (int k = 0; k < 3; ++k) {
            const float x = rs ? 0.f : th[k];                                       // cleared for the reset envs (:350-352)
            iv.thrusts[(3 * r + k) * N + e] = x;
            iv.forces[(3 * ModelIngenuity::sens_body[r] + k) * N + e] = x;
        }
    }
}

// post_physics_step (:356-365): progress++, observations, reward
template <class RED>
MI_HD void ing_post_env(const View& v, const IngenuityView& iv, const IngenuityParams& p, const int e0, const RED& red) {
    const int N = v.N;
    const bool valid = e0 < N;
    const int e = valid ? e0 : N - 1;
    float root[13], target[3];
    sfor<13>([&](auto K) MI_LAMBDA { root[K] = v.root[K * N + e]; });
    sfor<3>([&](auto K) MI_LAMBDA { target[K] = iv.target[K * N + e]; });
    const long long progress = v.progress[e] + 1;
    float obs[kIngObs], rew;
    long long reset;
    ingenuity_observations(root, target, obs);
    ingenuity_reward(root, target, root + 3, root + 10, progress, p.max_episode_length, &rew, &reset);
    red.episode(v, e, valid, rew, reset, progress);
    if (valid) store_step_outputs(v, e, obs, rew, reset, progress, p.max_episode_length);
}

// the task's own tensors of the __init__ state (:63-97): marker at the craft's default pose, target (0, 0, 1), zero thrusts
MI_HD void ing_init_env(const View& v, const IngenuityView& iv, const IngenuityParams& p, const int e) {
    const int N = v.N;
    for (int k = 0; k < 13; ++k) iv.marker[k * N + e] = (k == 2) ? p.init_height : (k == 6 ? 1.f : 0.f);
    for (int k = 0; k < 3; ++k) iv.target[k * N + e] = (k == 2) ? 1.f : 0.f;
    for (int k = 0; k < 3 * kIngRotors; ++k) iv.thrusts[k * N + e] = 0.f;
    for (int k = 0; k < 3 * kIngBodies; ++k) iv.forces[k * N + e] = 0.f;
}

}  // namespace mi
