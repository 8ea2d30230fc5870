// loco_step.hpp -- per-env bodies, host + device, of the tasks that live in step_kernels.hpp: the Cartpole post step and indexed reset, the
// indexed reset of Ant / Humanoid, and the tail every small task's post step ends with.  The kernels run them per lane, cpu/mi_engine_cpu.cpp
// per loop iteration (the layout of tasks/anymal_step.hpp).  A post body takes the job statistics through a reduction policy:
//     red.episode(v, e, valid, rew, reset, progress)
// On the device a wave reduction + one atomic per wave (step_kernels.hpp DevEpisodeRed), on the host a per-thread accumulator
// (cpu/cpu_engine.hpp HostEpisodeRed).  e0 >= N: a lane past the batch, which shadows env N - 1 and stores nothing, so that the device's wave
// reductions stay full; the host never passes one.
#pragma once
#include "../arena.hpp"
#include "locomotion.hpp"

namespace mi {

// what post_physics_step leaves behind for the caller: randomize_buf, the raw observations and their clipped copy in the ring slot, reward,
// reset flag, progress and the timeout mask (vec_task.py:389-399)
template <int NOBS>
MI_HD void store_step_outputs(const View& v, const int e, const float (&obs)[NOBS], const float rew, const long long reset, const long long progress,
                              const float max_episode_length) {
    v.randomize[e] += 1;
    float* ob = v.obs + (size_t)e * NOBS;
    float* oc = v.obs_out + ((size_t)v.ring * v.N + e) * NOBS;
    sfor<NOBS>([&](auto K) MI_LAMBDA { ob[K] = obs[K]; oc[K] = fminf(fmaxf(obs[K], -v.clip_obs), v.clip_obs); });
    v.rew[e] = rew;
    v.reset[e] = reset;
    v.progress[e] = progress;
    v.timeout[e] = (unsigned char)(((float)progress >= max_episode_length - 1.f) && (reset != 0));   // vec_task.py:394
}

// ------------------------------------------------------------------------------------------------ Cartpole
// post_physics_step (cartpole.py:165-174): progress++, reset if flagged, observations (:131-142), reward.  A shadow lane evaluates the reset
// too; only its stores are guarded.
template <class RED>
MI_HD void cartpole_post_env(const View& v, const CartpoleParams& tp, const int e0, const RED& red) {
    const int N = v.N;
    const bool valid = e0 < N;
    const int e = valid ? e0 : N - 1;
    float q[2] = {v.dof[e], v.dof[N + e]}, qd[2] = {v.dof[2 * N + e], v.dof[3 * N + e]};
    long long progress = v.progress[e] + 1;
    int ep = v.episode[e];
    if (v.reset[e] != 0) {
        cartpole_reset(v.seed, (uint32_t)(v.env_offset + e), (uint32_t)ep, q, qd);
        ep += 1;
        progress = 0;
        if (valid) sfor<2>([&](auto K) MI_LAMBDA { v.dof[K * N + e] = q[K]; v.dof[(2 + K) * N + e] = qd[K]; v.laml[K * N + e] = 0.f; });
    }
    float obs[4] = {q[0], qd[0], q[1], qd[1]};
    float rew;
    long long reset;
    cartpole_reward(tp, obs[2], obs[3], obs[1], obs[0], 0LL, progress, &rew, &reset);
    if (v.obs_noise.dist != 0)
        sfor<4>([&](auto K) MI_LAMBDA { obs[K] = apply_noise(v.obs_noise, v.seed, (uint32_t)(v.env_offset + e), v.step, 0u, (uint32_t)K, obs[K]); });
    red.episode(v, e, valid, rew, reset, progress);
    if (!valid) return;
    v.episode[e] = ep;
    store_step_outputs(v, e, obs, rew, reset, progress, tp.max_episode_length);
}
// reset_idx(env_ids) outside step(): the draws of the env's current episode number
MI_HD void cartpole_reset_env(const View& v, const int e) {
    const int N = v.N;
    float q[2], qd[2];
    const int ep = v.episode[e];
    cartpole_reset(v.seed, (uint32_t)(v.env_offset + e), (uint32_t)ep, q, qd);
    v.episode[e] = ep + 1;
    for (int k = 0; k < 2; ++k) { v.dof[k * N + e] = q[k]; v.dof[(2 + k) * N + e] = qd[k]; v.laml[k * N + e] = 0.f; }
    v.progress[e] = 0;
    v.reset[e] = 0;
}

// ------------------------------------------------------------------------------------------------ Ant / Humanoid
// reset_idx(env_ids) outside step() (ant.py:255-279)
template <class M, bool HUM>
MI_HD void loco_reset_env(const View& v, const LocoParams& tp, const int e) {
    using T = Loco<M::ND, 6 * M::NSENS, HUM>;
    const int N = v.N;
    float init_root[13], root[13], q[M::ND], qd[M::ND], pot, prev;
    for (int k = 0; k < 13; ++k) init_root[k] = v.init_root[k * N + e];
    const int ep = v.episode[e];
    T::reset(tp, v.seed, (uint32_t)(v.env_offset + e), (uint32_t)ep, init_root, root, q, qd, &pot, &prev);
    v.episode[e] = ep + 1;
    for (int k = 0; k < 13; ++k) v.root[k * N + e] = root[k];
    for (int k = 0; k < M::ND; ++k) { v.dof[k * N + e] = q[k]; v.dof[(M::ND + k) * N + e] = qd[k]; v.laml[k * N + e] = 0.f; }
    for (int k = 0; k < 3 * M::NSPH; ++k) v.lamc[k * N + e] = 0.f;
    if (M::NPG > 0 && v.lamp) for (int k = 0; k < 3 * M::NPG; ++k) v.lamp[k * N + e] = 0.f;
    v.potentials[e] = pot;
    v.prev_potentials[e] = prev;
    v.progress[e] = 0;
    v.reset[e] = 0;
}

}  // namespace mi
