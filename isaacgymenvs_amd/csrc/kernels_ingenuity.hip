// kernels_ingenuity.hip -- Ingenuity (reference isaacgymenvs/tasks/ingenuity.py): a free-flying chassis under Mars gravity with two
// coaxial rotors; the policy commands one thrust vector per rotor, applied on the rotor bodies in their local frames
// (apply_rigid_body_force_tensors, LOCAL_SPACE, :354).  pre kernel = pre_physics_step (periodic targets, deferred resets, thrusts),
// sub-step kernel = gym.simulate with the engine's Drive extras (zero gains: the joints are passive), post kernel =
// post_physics_step.  One env per lane, 64 envs per wave.
// The per-env bodies of the pre, post, init and reset kernels live in tasks/ingenuity_step.hpp, shared with the CPU backend
// (cpu/mi_engine_cpu.cpp); the kernels here are index arithmetic, a bounds check and one call.
#include "step_kernels.hpp"
#include "tasks/ingenuity_step.hpp"

namespace mi {

using IM = ModelIngenuity;
static_assert(IM::ND == kIngDof && IM::NSENS == kIngRotors && IM::NB + 1 == kIngBodies, "ingenuity model");

// pre_physics_step (:321-354)
__global__ void ing_pre_kernel(View v, IngenuityView iv, IngenuityParams p, const float* __restrict__ actions_in) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < v.N) ing_pre_env(v, iv, p, actions_in, e);
}

// gym.simulate(): one physics sub-step with the thrust vectors on the two rotor bodies
__global__ __launch_bounds__(64) void ing_substep_kernel(View v, IngenuityView iv, SimParams P, IngenuityParams p) {
    extern __shared__ float lds_rows[];
    using S = Sim<IM>;
    static_assert(S::LANES == 64, "ingenuity uses the static row store");
    const int e = blockIdx.x * 64 + threadIdx.x;
    const int N = v.N;
    if (e >= N) return;
    S sim;
    load_sim(sim, v, e);
    float tau[kIngDof], target[kIngDof], fs[kIngRotors][3];
    sfor<kIngDof>([&](auto K) MI_LAMBDA { tau[K] = 0.f; target[K] = 0.f; });
    sfor<kIngRotors>([&](auto R) MI_LAMBDA { sfor<3>([&](auto K) MI_LAMBDA { fs[R][K] = iv.forces[(3 * IM::sens_body[R] + K) * N + e]; }); });
    const Drive drv{0.f, 0.f, target, &fs[0][0]};                                   // stiffness = damping = 0 (:264-267)
    const float h = P.dt / (float)P.substeps;
    sim.substep(P, tau, h, RowStore<64>(lds_rows + threadIdx.x), Strided{v.lamc + e, N}, Strided{v.laml + e, N}, Strided{v.sensor + e, N},
                Strided{v.dof_force + e, N}, PlaneGround{}, -1.f, Strided{nullptr, N}, &drv);
    // asset_options.max_angular_velocity (:248): PhysX clamps the angular speed of the body
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

// post_physics_step (:356-365)
__global__ __launch_bounds__(64) void ing_post_kernel(View v, IngenuityView iv, IngenuityParams p) {
    ing_post_env(v, iv, p, (int)(blockIdx.x * 64 + threadIdx.x), DevEpisodeRed{});
}

// __init__ state (:63-97) after init_state_kernel: marker at the default pose, target (0, 0, 1), zero thrusts
__global__ void ing_init_kernel(View v, IngenuityView iv, IngenuityParams p) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < v.N) ing_init_env(v, iv, p, e);
}
__global__ void ing_reset_ids_kernel(View v, IngenuityView iv, IngenuityParams p, const long long* __restrict__ ids, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int e = (int)ids[i];
    if (e >= 0 && e < v.N) ing_reset_env(v, iv, p, e, v.episode[e]);
}

static hipError_t ing_substeps(const View& v, const IngenuityView& iv, const SimParams& P, const IngenuityParams& p, int n, hipStream_t s) {
    constexpr size_t lds = lds_bytes<IM>();
    static unsigned long long configured = 0ull;
    if (hipError_t e = ensure_dynamic_lds((const void*)ing_substep_kernel, lds, &configured); e != hipSuccess) return e;
    for (int i = 0; i < n; ++i) hipLaunchKernelGGL(ing_substep_kernel, dim3((v.N + 63) / 64), dim3(64), lds, s, v, iv, P, p);
    return hipGetLastError();
}
hipError_t launch_step_ingenuity(const View& v, const IngenuityView& iv, const SimParams& P, const IngenuityParams& p, const float* actions,
                                 int cfi, hipStream_t s) {
    hipLaunchKernelGGL(ing_pre_kernel, dim3((v.N + 63) / 64), dim3(64), 0, s, v, iv, p, actions);
    hipError_t e = ing_substeps(v, iv, P, p, cfi * P.substeps, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ing_post_kernel, dim3((v.N + 63) / 64), dim3(64), 0, s, v, iv, p);
    return hipGetLastError();
}
hipError_t launch_simulate_ingenuity(const View& v, const IngenuityView& iv, const SimParams& P, const IngenuityParams& p, hipStream_t s) {
    return ing_substeps(v, iv, P, p, P.substeps, s);
}
hipError_t launch_init_ingenuity(const View& v, const IngenuityView& iv, const IngenuityParams& p, hipStream_t s) {
    hipLaunchKernelGGL(ing_init_kernel, dim3((v.N + 127) / 128), dim3(128), 0, s, v, iv, p);
    return hipGetLastError();
}
hipError_t launch_reset_ingenuity(const View& v, const IngenuityView& iv, const IngenuityParams& p, const long long* ids, int n, hipStream_t s) {
    hipLaunchKernelGGL(ing_reset_ids_kernel, dim3((n + 127) / 128), dim3(128), 0, s, v, iv, p, ids, n);
    return hipGetLastError();
}

}  // namespace mi
