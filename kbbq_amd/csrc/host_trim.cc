// host_trim.cc -- the host side of trimming and filtering (include/kbbq_engine.h: kbbq_trim_ee_table, kbbq_trim_ee_bound):
// the expected-error table the kernel sums and the conversion of a bound given in expected errors.  No GPU is touched.
//
// EE[v] = round(10^(-v/10) * 2^32), built in long double: no 10^(-v/10) * 2^32 for v <= 93 lies within 0.003 of a half, so
// any sane powl gives the same integers (EE[0] = 4294967296, EE[10] = 429496730, EE[20] = 42949673, EE[30] = 4294967,
// EE[93] = 2).  Above 93 the values are 1 or 0 (v >= 97): a quality pass 4 never writes.
#include <cmath>
#include <cstdint>

#include "host_text.h"      // (for kbbq_fail alone)

extern "C" {

int kbbq_trim_ee_table(uint64_t out[256]) {
    if (!out) return kbbq_fail(KBBQ_EINVAL, "null argument");
    for (int v = 0; v < 256; ++v) out[v] = (uint64_t)roundl(powl(10.0L, -(long double)v / 10.0L) * 4294967296.0L);
    return KBBQ_OK;
}

int kbbq_trim_ee_bound(double max_ee, uint64_t *bound) {
    if (!bound) return kbbq_fail(KBBQ_EINVAL, "null argument");
    // (not > 0 also catches a NaN)
    if (!(max_ee > 0) || !(max_ee < 4294967296.0)) return kbbq_fail(KBBQ_EINVAL, "max_ee must be above 0 and below 2^32");
    *bound = (uint64_t)floorl((long double)max_ee * 4294967296.0L);      // (exact: a double times a power of two)
    return KBBQ_OK;
}

}  // extern "C"
