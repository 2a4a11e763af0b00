// tools/trim_host_check.cc -- the host code of trimming as a stand-alone program, to be built with a sanitizer on the CPU:
// the values of --trim-tail, --min-length and --max-ee from their text (kbbq_amd/csrc/trim_values.h), the conversion of a bound
// in expected errors and the expected-error table (kbbq_amd/csrc/host_trim.cc).  No GPU, no engine library.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o trim_host_check tools/trim_host_check.cc kbbq_amd/csrc/host_trim.cc
//   ./trim_host_check            (prints "trim host check: ok"; any finding or wrong value ends it with a message and status 1)
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../kbbq_amd/csrc/trim_values.h"

// host_trim.cc reports through the library's kbbq_fail; here it only keeps the text
static char g_text[256];
int kbbq_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_text, sizeof g_text, fmt, ap);
    va_end(ap);
    return code;
}

static int g_bad = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_bad; } \
    } while (0)

int main() {
    // ---- the table
    uint64_t ee[256];
    CHECK(kbbq_trim_ee_table(ee) == KBBQ_OK);
    CHECK(ee[0] == 4294967296ull && ee[10] == 429496730ull && ee[20] == 42949673ull && ee[30] == 4294967ull && ee[93] == 2ull);
    for (int v = 1; v < 256; ++v) CHECK(ee[v] <= ee[v - 1]);
    CHECK(ee[255] == 0);
    CHECK(kbbq_trim_ee_table(nullptr) == KBBQ_EINVAL);
    // 8 388 607 bases of quality 0 stay below 2^56
    CHECK(ee[0] * 8388607ull < (1ull << 56));
    // ---- the bound
    uint64_t b = 0;
    CHECK(kbbq_trim_ee_bound(2.0, &b) == KBBQ_OK && b == (2ull << 32));
    CHECK(kbbq_trim_ee_bound(0.1, &b) == KBBQ_OK && b == 429496729ull);
    CHECK(kbbq_trim_ee_bound(1.0 / 4294967296.0, &b) == KBBQ_OK && b == 1);
    CHECK(kbbq_trim_ee_bound(0.5 / 4294967296.0, &b) == KBBQ_OK && b == 0);
    CHECK(kbbq_trim_ee_bound(4294967295.999, &b) == KBBQ_OK && b > (1ull << 63));
    const double bad_bounds[] = {0.0, -0.0, -1.0, 4294967296.0, 1e300, -1e300, std::nan(""), HUGE_VAL, -HUGE_VAL};
    for (double x : bad_bounds) CHECK(kbbq_trim_ee_bound(x, &b) == KBBQ_EINVAL);
    CHECK(kbbq_trim_ee_bound(1.0, nullptr) == KBBQ_EINVAL);
    // ---- integers
    uint64_t v = 0;
    CHECK(trim_parse_integer("1", 1, 93, &v) && v == 1);
    CHECK(trim_parse_integer("93", 1, 93, &v) && v == 93);
    CHECK(trim_parse_integer("0093", 1, 93, &v) && v == 93);
    CHECK(trim_parse_integer("8388607", 1, 8388607, &v) && v == 8388607);
    CHECK(trim_parse_integer("18446744073709551615", 0, UINT64_MAX, &v) && v == UINT64_MAX);
    const char *bad_ints[] = {"", "0", "94", "-1", "+5", " 5", "5 ", "5.0", "1e1", "0x10", "five", "18446744073709551616", "99999999999999999999999999", "9\n"};
    for (const char *t : bad_ints) CHECK(!trim_parse_integer(t, 1, 93, &v));
    CHECK(!trim_parse_integer(nullptr, 1, 93, &v));
    // ---- decimals
    double e = 0;
    CHECK(trim_parse_max_ee("2", &e, &b) && e == 2.0 && b == (2ull << 32));
    CHECK(trim_parse_max_ee("0.5", &e, &b) && b == (1ull << 31));
    CHECK(trim_parse_max_ee(".25", &e, &b) && b == (1ull << 30));
    CHECK(trim_parse_max_ee("1e-3", &e, &b) && b == 4294967ull);
    CHECK(trim_parse_max_ee("2.5E+0", &e, &b) && b == (5ull << 31));
    const char *bad_ees[] = {"", "0", "0.0", "-1", "+1", " 1", "1 ", "1e", "e5", "nan", "inf", "infinity", "0x2", "two", "1,5", "4294967296", "1e400", "1e-400", "1..2", "--1", "1e5e5"};
    for (const char *t : bad_ees) CHECK(!trim_parse_max_ee(t, &e, &b));
    CHECK(!trim_parse_max_ee(nullptr, &e, &b));
    // a long argument is read to its end and no further
    std::string nines(5000, '9');
    CHECK(!trim_parse_integer(nines.c_str(), 1, 93, &v));
    CHECK(!trim_parse_max_ee(nines.c_str(), &e, &b));
    if (g_bad) { fprintf(stderr, "trim host check: %d failed\n", g_bad); return 1; }
    printf("trim host check: ok\n");
    return 0;
}
