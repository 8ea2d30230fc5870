// kernels_ball_balance.hip -- BallBalance (reference isaacgymenvs/tasks/ball_balance.py): a tray on three position-driven legs
// keeps a dropped ball in place.  pre kernel = pre_physics_step (deferred resets, position targets), sub-step kernel =
// gym.simulate on core/bbot_engine.hpp (attractor-pinned feet, ball <-> tray contact), post kernel = post_physics_step.
// One env per lane, 64 envs per wave; the sub-step keeps its 18 constraint rows in registers (no LDS).
// The per-env bodies of the pre, post, init and reset kernels live in tasks/ball_balance_step.hpp, shared with the CPU backend
// (cpu/mi_engine_cpu.cpp); the kernels here are index arithmetic, a bounds check and one call.
#include "step_kernels.hpp"
#include "core/bbot_engine.hpp"
#include "tasks/ball_balance_step.hpp"

namespace mi {

using BM = ModelBalanceBot;
static_assert(BM::ND == kBbotDof && BM::NSENS == kBbotSensors && BM::NB == 7, "balance bot model");
static_assert(sizeof(BbotPhys) == sizeof(BallBalanceParams) - offsetof(BallBalanceParams, pin_stiffness), "BbotPhys is the tail of BallBalanceParams");

static __device__ __forceinline__ const BbotPhys& phys_of(const BallBalanceParams& p) { return *reinterpret_cast<const BbotPhys*>(&p.pin_stiffness); }

// pre_physics_step (:395-413)
__global__ void bbot_pre_kernel(View v, BbotView bv, BallBalanceParams p, const float* __restrict__ actions_in) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < v.N) bbot_pre_env(v, bv, p, actions_in, e);
}

// gym.simulate(): one physics sub-step
__global__ __launch_bounds__(64) void bbot_substep_kernel(View v, BbotView bv, SimParams P, BallBalanceParams p) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    const int N = v.N;
    if (e >= N) return;
    BbotSim<BM> sim;
    load_sim(sim, v, e);
    float target[kBbotDof];
    sfor<kBbotDof>([&](auto K) MI_LAMBDA { target[K] = bv.targets[K * N + e]; });
    sfor<3>([&](auto K) MI_LAMBDA { sim.ball.pos[K] = bv.ball[K * N + e]; sim.ball.vel[K] = bv.ball[(7 + K) * N + e]; sim.ball.angvel[K] = bv.ball[(10 + K) * N + e]; });
    sfor<4>([&](auto K) MI_LAMBDA { sim.ball.quat[K] = bv.ball[(3 + K) * N + e]; });
    int nc;
    sim.substep(P, phys_of(p), P.dt / (float)P.substeps, target, Strided{v.laml + e, N}, Strided{bv.lamp + e, N}, Strided{v.sensor + e, N}, &nc);
    bv.ncontact[e] = nc;
    store_sim(sim, v, e);
    sfor<3>([&](auto K) MI_LAMBDA { bv.ball[K * N + e] = sim.ball.pos[K]; bv.ball[(7 + K) * N + e] = sim.ball.vel[K]; bv.ball[(10 + K) * N + e] = sim.ball.angvel[K]; });
    sfor<4>([&](auto K) MI_LAMBDA { bv.ball[(3 + K) * N + e] = sim.ball.quat[K]; });
}

// post_physics_step (:415-424)
__global__ __launch_bounds__(64) void bbot_post_kernel(View v, BbotView bv, BallBalanceParams p) {
    bbot_post_env(v, bv, p, (int)(blockIdx.x * 64 + threadIdx.x), DevEpisodeRed{});
}

// __init__ state (:88-112) after init_state_kernel: ball at its spawn pose, zero targets
__global__ void bbot_init_kernel(View v, BbotView bv, BallBalanceParams p) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < v.N) bbot_init_env(v, bv, p, e);
}
__global__ void bbot_reset_ids_kernel(View v, BbotView bv, BallBalanceParams p, const long long* __restrict__ ids, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int e = (int)ids[i];
    if (e < 0 || e >= v.N) return;
    bbot_reset_env(v, bv, p, e);
    for (int d = 0; d < kBbotDof; ++d) bv.targets[d * v.N + e] = 0.f;          // the pre step's `rs ? 0 : t`
}

static hipError_t bbot_substeps(const View& v, const BbotView& bv, const SimParams& P, const BallBalanceParams& p, int n, hipStream_t s) {
    for (int i = 0; i < n; ++i) hipLaunchKernelGGL(bbot_substep_kernel, dim3((v.N + 63) / 64), dim3(64), 0, s, v, bv, P, p);
    return hipGetLastError();
}
hipError_t launch_step_ball_balance(const View& v, const BbotView& bv, const SimParams& P, const BallBalanceParams& p, const float* actions,
                                    int cfi, hipStream_t s) {
    hipLaunchKernelGGL(bbot_pre_kernel, dim3((v.N + 63) / 64), dim3(64), 0, s, v, bv, p, actions);
    hipError_t e = bbot_substeps(v, bv, P, p, cfi * P.substeps, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bbot_post_kernel, dim3((v.N + 63) / 64), dim3(64), 0, s, v, bv, p);
    return hipGetLastError();
}
hipError_t launch_simulate_ball_balance(const View& v, const BbotView& bv, const SimParams& P, const BallBalanceParams& p, hipStream_t s) {
    return bbot_substeps(v, bv, P, p, P.substeps, s);
}
hipError_t launch_init_ball_balance(const View& v, const BbotView& bv, const BallBalanceParams& p, hipStream_t s) {
    hipLaunchKernelGGL(bbot_init_kernel, dim3((v.N + 127) / 128), dim3(128), 0, s, v, bv, p);
    return hipGetLastError();
}
hipError_t launch_reset_ball_balance(const View& v, const BbotView& bv, const BallBalanceParams& p, const long long* ids, int n, hipStream_t s) {
    hipLaunchKernelGGL(bbot_reset_ids_kernel, dim3((n + 127) / 128), dim3(128), 0, s, v, bv, p, ids, n);
    return hipGetLastError();
}

}  // namespace mi
