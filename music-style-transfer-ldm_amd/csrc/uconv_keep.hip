// dec1's launches with the regional keep (EPI_KEEP, guided or not): uconv.hip's templates compiled into a code object of
// their own, see step_dec1_keep there.
#define UCONV_KEEP_TU 1
#include "uconv.hip"
