// Host (g++) build of the block sweeps' weight selection (csrc/core/engine_mw.hpp sweep_weights) -- TEST-ONLY (tests/test_mw_sweep_weights.py).
#include "../../isaacgymenvs_amd/csrc/core/engine.hpp"
#include "../../isaacgymenvs_amd/csrc/core/engine_mw.hpp"

// out[0], out[1]: om and iom as substep_role selects them; out[2], out[3]: the arithmetic they replace, the division done at run time
extern "C" void hs_sweep_weights(float nact, float* out) {
    mi::sweep_weights(nact, out[0], out[1]);
    volatile float n = nact, one = 1.f;
    const float nn = n;
    const float om = (nn > 1.5f) ? 0.5f * (nn + 1.f) : 1.f;
    out[2] = om;
    volatile float d = om;
    out[3] = one / d;
}
