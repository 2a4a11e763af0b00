// host_adapter.cc -- the host side of 3' adapter removal (include/kbbq_engine.h: kbbq_adapter_parse): an adapter from its text,
// a sequence or one of three names, in the 2-bit layout the kernel compares against.  No GPU is touched.
#include <cstdint>
#include <cstring>
#include <strings.h>

#include "host_text.h"      // (for kbbq_fail alone)

extern "C" {

int kbbq_adapter_parse(const char *text, kbbq_adapter *out) {
    if (!text || !out) return kbbq_fail(KBBQ_EINVAL, "null argument");
    static const char *const named[][2] = {
        {"illumina", "AGATCGGAAGAGC"}, {"nextera", "CTGTCTCTTATACACATCT"}, {"smallrna", "TGGAATTCTCGGGTGCCAAGG"}};
    for (const auto &n : named)
        if (!strcasecmp(text, n[0])) text = n[1];
    const size_t len = strlen(text);
    if (len < KBBQ_ADAPTER_MIN || len > KBBQ_ADAPTER_MAX)
        return kbbq_fail(KBBQ_EINVAL, "an adapter is %d to %d letters of ACGT, or illumina, nextera or smallrna", KBBQ_ADAPTER_MIN, KBBQ_ADAPTER_MAX);
    kbbq_adapter a = {{0, 0}, (int32_t)len, 0};
    for (size_t j = 0; j < len; ++j) {
        uint64_t code;
        switch (text[j]) {
        case 'A': case 'a': code = 0; break;
        case 'C': case 'c': code = 1; break;
        case 'G': case 'g': code = 2; break;
        case 'T': case 't': code = 3; break;
        default: return kbbq_fail(KBBQ_EINVAL, "an adapter is %d to %d letters of ACGT, or illumina, nextera or smallrna", KBBQ_ADAPTER_MIN, KBBQ_ADAPTER_MAX);
        }
        a.code[j / 32] |= code << (2 * (j % 32));
    }
    *out = a;
    return KBBQ_OK;
}

}  // extern "C"
