// dec1's launches with the regional keep (EPI_KEEP, guided or not) in a code object of their own, like the guided
// loop's (uconv_guide.hip, uconv_kernel.h).
#include "uconv_kernel.h"

namespace ldm {
namespace uc {

int step_dec1_keep(int geo, const UArgs& a, const StepConv& s, hipStream_t st) {
    LDM_REQUIRE(s.xs && s.coef && !s.plain, "dec1 (keep): sampler state, coefficients");
    return dec1_visit(geo, [&](auto g) -> int {
        constexpr int GEO = decltype(g)::value;
        if (s.guide_eb) {
            if (s.msolver) return dec1_launch<EPI_MSOLVER | EPI_GUIDE | EPI_KEEP, GEO>(a, s.dtype, st);
            return dec1_launch<EPI_DDIM | EPI_GUIDE | EPI_KEEP, GEO>(a, s.dtype, st);
        }
        if (s.msolver) return dec1_launch<EPI_MSOLVER | EPI_KEEP, GEO>(a, s.dtype, st);
        return dec1_launch<EPI_DDIM | EPI_KEEP, GEO>(a, s.dtype, st);
    });
}

}  // namespace uc
}  // namespace ldm
