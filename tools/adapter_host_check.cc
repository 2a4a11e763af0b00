// tools/adapter_host_check.cc -- the host code of 3' adapter removal as a stand-alone program, to be built with a sanitizer on
// the CPU: an adapter from its text (kbbq_amd/csrc/host_adapter.cc) and the value of --adapter-error-rate from its text
// (kbbq_amd/csrc/adapter_values.h).  No GPU, no engine library.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o adapter_host_check tools/adapter_host_check.cc kbbq_amd/csrc/host_adapter.cc
//   ./adapter_host_check            (prints "adapter host check: ok"; any finding or wrong value ends it with a message and status 1)
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

#include "../include/kbbq_engine.h"
#include "../kbbq_amd/csrc/adapter_values.h"

// host_adapter.cc reports through the library's kbbq_fail; here it only keeps the text
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
    kbbq_adapter a;
    // names in any case are their sequences
    const char *named[][2] = {{"illumina", "AGATCGGAAGAGC"}, {"NEXTERA", "CTGTCTCTTATACACATCT"}, {"SmallRNA", "TGGAATTCTCGGGTGCCAAGG"}};
    for (auto &n : named) {
        kbbq_adapter b;
        CHECK(kbbq_adapter_parse(n[0], &a) == KBBQ_OK && kbbq_adapter_parse(n[1], &b) == KBBQ_OK);
        CHECK(a.len == (int32_t)strlen(n[1]) && a.len == b.len && a.code[0] == b.code[0] && a.code[1] == b.code[1] && a.reserved == 0);
    }
    // the layout: base j in bits 2(j%32).. of word j/32, A C G T = 0 1 2 3, either case, nothing behind the last base
    CHECK(kbbq_adapter_parse("ACGT", &a) == KBBQ_OK && a.len == 4 && a.code[0] == 0xE4 && a.code[1] == 0);
    CHECK(kbbq_adapter_parse("acgt", &a) == KBBQ_OK && a.code[0] == 0xE4);
    const std::string t64(64, 'T'), t33 = std::string(32, 'A') + "G", t65(65, 'T');
    CHECK(kbbq_adapter_parse(t64.c_str(), &a) == KBBQ_OK && a.len == 64 && a.code[0] == ~0ULL && a.code[1] == ~0ULL);
    CHECK(kbbq_adapter_parse(t33.c_str(), &a) == KBBQ_OK && a.len == 33 && a.code[0] == 0 && a.code[1] == 2);
    // what is refused leaves the output alone
    a.len = -7;
    for (const char *bad : {"", "ACG", "ACGN", "ACGTN", "ACGU", "AC GT", "illumin", "truseq", "ACGT\n", t65.c_str()})
        CHECK(kbbq_adapter_parse(bad, &a) == KBBQ_EINVAL && a.len == -7);
    CHECK(kbbq_adapter_parse(nullptr, &a) == KBBQ_EINVAL && kbbq_adapter_parse("ACGT", nullptr) == KBBQ_EINVAL);

    int32_t v = -1;
    const struct { const char *text; int32_t want; } rates[] = {{"0", 0}, {"0.1", 100}, {".125", 125}, {"0.5", 500}, {"0.500", 500}, {"0.", 0},
                                                               {"0.05", 50}, {"0.001", 1}, {"00.2", 200}, {"0.10", 100}};
    for (auto &r : rates) CHECK(adapter_parse_error_rate(r.text, &v) && v == r.want);
    v = -1;
    for (const char *bad : {"", ".", "0.501", "0.6", "1", "1.0", "10", "0.1234", "0.0625", "1e-1", "-0.1", "+0.1", " 0.1", "0.1 ", "0,1", "nan", "0x0",
                            "99999999999999999999999"})
        CHECK(!adapter_parse_error_rate(bad, &v) && v == -1);
    CHECK(!adapter_parse_error_rate(nullptr, &v));

    if (g_bad) return 1;
    puts("adapter host check: ok");
    return 0;
}
