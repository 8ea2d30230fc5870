// kernels_quadcopter.hip -- Quadcopter (reference isaacgymenvs/tasks/quadcopter.py): free-flying chassis with four tilting
// rotors; position-driven rotor joints (DOF_MODE_POS) and thrust forces on the rotor bodies (apply_rigid_body_force_tensors,
// LOCAL_SPACE).  pre kernel = pre_physics_step (deferred resets, action integration), sub-step kernel = gym.simulate with the
// engine's Drive extras, post kernel = post_physics_step.  One env per lane, 64 envs per wave.
// The per-env bodies of the pre, post, init and reset kernels live in tasks/quadcopter_step.hpp, shared with the CPU backend
// (cpu/mi_engine_cpu.cpp); the kernels here are index arithmetic, a bounds check and one call.
#include "step_kernels.hpp"
#include "tasks/quadcopter_step.hpp"

namespace mi {

using QM = ModelQuadcopter;
static_assert(QM::ND == kQuadDof && QM::NSENS == kQuadRotors && QM::NB == 9, "quadcopter model");

// pre_physics_step (quadcopter.py:276-292)
__global__ void quad_pre_kernel(View v, QuadView qv, QuadcopterParams p, const float* __restrict__ actions_in) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < v.N) quad_pre_env(v, qv, p, actions_in, e);
}

// gym.simulate(): one physics sub-step with the position drives and the rotor thrusts
__global__ __launch_bounds__(64) void quad_substep_kernel(View v, QuadView qv, SimParams P, QuadcopterParams p) {
    extern __shared__ float lds_rows[];
    using S = Sim<QM>;
    static_assert(S::LANES == 64, "quadcopter uses the static row store");
    const int e = blockIdx.x * 64 + threadIdx.x;
    const int N = v.N;
    if (e >= N) return;
    S sim;
    load_sim(sim, v, e);
    float tau[kQuadDof], target[kQuadDof], fs[kQuadRotors][3];
    sfor<kQuadDof>([&](auto K) MI_LAMBDA { tau[K] = 0.f; target[K] = qv.targets[K * N + e]; });
    sfor<kQuadRotors>([&](auto K) MI_LAMBDA { fs[K][0] = 0.f; fs[K][1] = 0.f; fs[K][2] = qv.forces[(3 * QM::sens_body[K] + 2) * N + e]; });
    const Drive drv{p.drive_stiffness, p.drive_damping, target, &fs[0][0]};
    const float h = P.dt / (float)P.substeps;
    sim.substep(P, tau, h, RowStore<64>(lds_rows + threadIdx.x), Strided{v.lamc + e, N}, Strided{v.laml + e, N}, Strided{v.sensor + e, N},
                Strided{v.dof_force + e, N}, PlaneGround{}, -1.f, Strided{nullptr, N}, &drv);
    // asset_options.max_angular_velocity (:208): PhysX clamps the angular speed of the body
    {
        const float w2 = sim.root[10] * sim.root[10] + sim.root[11] * sim.root[11] + sim.root[12] * sim.root[12];
        const float lim = p.max_angular_velocity;
        if (w2 > lim * lim) {
            const float sc = lim * MI_RSQ(w2);
            sim.root[10] *= sc; sim.root[11] *= sc; sim.root[12] *= sc;
        }
    }
    store_sim(sim, v, e);
}

// post_physics_step (:294-302)
__global__ __launch_bounds__(64) void quad_post_kernel(View v, QuadView qv, QuadcopterParams p) {
    quad_post_env(v, qv, p, (int)(blockIdx.x * 64 + threadIdx.x), DevEpisodeRed{});
}

// __init__ state (:62-101) after init_state_kernel: zero targets / thrusts
__global__ void quad_init_kernel(View v, QuadView qv, QuadcopterParams p) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < v.N) quad_init_env(v, qv, p, e);
}
__global__ void quad_reset_ids_kernel(View v, QuadView qv, QuadcopterParams p, const long long* __restrict__ ids, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int e = (int)ids[i];
    float q[kQuadDof];
    if (e >= 0 && e < v.N) quad_reset_env(v, qv, p, e, q);
}

static hipError_t quad_substeps(const View& v, const QuadView& qv, const SimParams& P, const QuadcopterParams& p, int n, hipStream_t s) {
    constexpr size_t lds = lds_bytes<QM>();
    static unsigned long long configured = 0ull;
    if (hipError_t e = ensure_dynamic_lds((const void*)quad_substep_kernel, lds, &configured); e != hipSuccess) return e;
    for (int i = 0; i < n; ++i) hipLaunchKernelGGL(quad_substep_kernel, dim3((v.N + 63) / 64), dim3(64), lds, s, v, qv, P, p);
    return hipGetLastError();
}
hipError_t launch_step_quadcopter(const View& v, const QuadView& qv, const SimParams& P, const QuadcopterParams& p, const float* actions,
                                  int cfi, hipStream_t s) {
    // 64-thread blocks like the sub-step kernel: block b of every kernel of the step lands on the same XCD (own L2)
    hipLaunchKernelGGL(quad_pre_kernel, dim3((v.N + 63) / 64), dim3(64), 0, s, v, qv, p, actions);
    hipError_t e = quad_substeps(v, qv, P, p, cfi * P.substeps, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(quad_post_kernel, dim3((v.N + 63) / 64), dim3(64), 0, s, v, qv, p);
    return hipGetLastError();
}
hipError_t launch_simulate_quadcopter(const View& v, const QuadView& qv, const SimParams& P, const QuadcopterParams& p, hipStream_t s) {
    return quad_substeps(v, qv, P, p, P.substeps, s);
}
hipError_t launch_init_quadcopter(const View& v, const QuadView& qv, const QuadcopterParams& p, hipStream_t s) {
    hipLaunchKernelGGL(quad_init_kernel, dim3((v.N + 127) / 128), dim3(128), 0, s, v, qv, p);
    return hipGetLastError();
}
hipError_t launch_reset_quadcopter(const View& v, const QuadView& qv, const QuadcopterParams& p, const long long* ids, int n, hipStream_t s) {
    hipLaunchKernelGGL(quad_reset_ids_kernel, dim3((n + 127) / 128), dim3(128), 0, s, v, qv, p, ids, n);
    return hipGetLastError();
}

// stand-alone replacement of the jitted function (row-major contiguous tensors)
__global__ void quadcopter_reward_kernel(int n, const float* root_positions, const float* root_quats, const float* root_linvels,
                                         const float* root_angvels, const long long* progress_buf, float max_episode_length, float* rew,
                                         long long* reset) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    float root[13];
    for (int k = 0; k < 3; ++k) { root[k] = root_positions[3 * (size_t)e + k]; root[7 + k] = root_linvels[3 * (size_t)e + k]; root[10 + k] = root_angvels[3 * (size_t)e + k]; }
    for (int k = 0; k < 4; ++k) root[3 + k] = root_quats[4 * (size_t)e + k];
    quadcopter_reward(root, progress_buf[e], max_episode_length, rew + e, reset + e);
}
hipError_t launch_quadcopter_reward(int n, const float* root_positions, const float* root_quats, const float* root_linvels,
                                    const float* root_angvels, const long long* progress_buf, float max_episode_length, float* rew,
                                    long long* reset, hipStream_t s) {
    hipLaunchKernelGGL(quadcopter_reward_kernel, dim3((n + 127) / 128), dim3(128), 0, s, n, root_positions, root_quats, root_linvels,
                       root_angvels, progress_buf, max_episode_length, rew, reset);
    return hipGetLastError();
}

}  // namespace mi
