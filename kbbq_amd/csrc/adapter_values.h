// adapter_values.h -- the value of --adapter-error-rate from its text (cli_options.h): a decimal of at most three places in
// 0..0.5, read digit by digit into permille -- no double in between, so that 0.1 is 100 and nothing else.  Plain host code, so that a stand-alone program can run it under a sanitizer
// (tools/adapter_host_check.cc).
#pragma once
#include <cstdint>

// "0", "0.1", ".125", "0.5", "0.500": digits, at most one point, at most three digits behind it, at least one digit in all, the
// value at most 0.5; false: not one
static bool adapter_parse_error_rate(const char *text, int32_t *permille) {
    if (!text || !*text) return false;
    const char *p = text;
    uint64_t whole = 0;
    int whole_digits = 0, places = 0;
    for (; *p >= '0' && *p <= '9'; ++p, ++whole_digits)
        if ((whole = whole * 10 + (uint64_t)(*p - '0')) > 1) return false;      // (0.5 at the most: the whole part is 0)
    uint32_t frac = 0;
    if (*p == '.') {
        for (++p; *p >= '0' && *p <= '9'; ++p, ++places) {
            if (places >= 3) return false;
            frac = frac * 10 + (uint32_t)(*p - '0');
        }
    }
    if (*p || whole_digits + places == 0) return false;
    for (int i = places; i < 3; ++i) frac *= 10;
    const uint64_t v = whole * 1000 + frac;
    if (v > 500) return false;
    *permille = (int32_t)v;
    return true;
}
