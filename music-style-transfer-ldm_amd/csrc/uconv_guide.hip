// dec1's launches of the guided reverse loop (EPI_GUIDE and the plain base half) in a code object of their own, so that
// the unguided step kernels' code object holds exactly the instances it held without guidance (uconv_kernel.h).
#include "uconv_kernel.h"

namespace ldm {
namespace uc {

// on geometry geo: the base half as a plain conv, or the target half with the guided DDIM / multistep update
int step_dec1_guided(int geo, const UArgs& a, const StepConv& s, hipStream_t st) {
    return dec1_visit(geo, [&](auto g) -> int {
        constexpr int GEO = decltype(g)::value;
        if (s.plain) return dec1_launch<0, GEO>(a, s.dtype, st);
        LDM_REQUIRE(s.xs && s.coef, "dec1 (guided): sampler state, coefficients");
        if (s.msolver) return dec1_launch<EPI_MSOLVER | EPI_GUIDE, GEO>(a, s.dtype, st);
        return dec1_launch<EPI_DDIM | EPI_GUIDE, GEO>(a, s.dtype, st);
    });
}

}  // namespace uc
}  // namespace ldm
