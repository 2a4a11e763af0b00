// trim_values.h -- the values of --trim-tail, --min-length and --max-ee from their text (cli_options.h): whole, in range, and
// nothing behind the number.  Plain host code over include/kbbq_engine.h's kbbq_trim_ee_bound, so that a stand-alone program
// can run it under a sanitizer (tools/trim_host_check.cc).
#pragma once
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "../../include/kbbq_engine.h"

// a decimal integer in lo..hi and nothing else (no sign, no blank, no exponent); false: not one
static bool trim_parse_integer(const char *text, uint64_t lo, uint64_t hi, uint64_t *out) {
    if (!text || !*text) return false;
    uint64_t v = 0;
    for (const char *p = text; *p; ++p) {
        if (*p < '0' || *p > '9') return false;
        if (v > (UINT64_MAX - (uint64_t)(*p - '0')) / 10) return false;
        v = v * 10 + (uint64_t)(*p - '0');
    }
    if (v < lo || v > hi) return false;
    *out = v;
    return true;
}

// a decimal number above 0 whose bound fits (kbbq_trim_ee_bound: below 2^32), and nothing else; false: not one
static bool trim_parse_max_ee(const char *text, double *value, uint64_t *bound) {
    if (!text || !*text || !((*text >= '0' && *text <= '9') || *text == '.')) return false;      // (strtod would take blanks, signs, "inf", "nan", "0x")
    for (const char *p = text; *p; ++p)
        if (!((*p >= '0' && *p <= '9') || *p == '.' || *p == 'e' || *p == 'E' || *p == '-' || *p == '+')) return false;
    char *end = nullptr;
    errno = 0;
    const double v = strtod(text, &end);
    if (end == text || *end || errno == ERANGE || !std::isfinite(v)) return false;
    if (kbbq_trim_ee_bound(v, bound) < 0) return false;
    *value = v;
    return true;
}
