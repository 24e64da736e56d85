// dec1's launches of the guided reverse loop (EPI_GUIDE and the plain base half): uconv.hip's templates compiled into a
// code object of their own, see step_dec1_guided there.
#define UCONV_GUIDE_TU 1
#include "uconv.hip"
