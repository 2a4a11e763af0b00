// cli_pair_walk.h -- which reads of which batches are mates: the one walk over a paired input's batches that --pair-overlap and
// --pair-correct share (cli_trim.h).  Plain host code over the batches' read counts, nothing of the GPU in it, so that the CPU
// suite reaches it (cli_io_test.h: --io-test pair-runs).
//
// Two files: pair j is record j of either, and the two files' batches are cut where their own bytes say -- the runs are the
// intersections of the two partitions.  Interleaved: record 2j and record 2j + 1 are mates, and a batch may begin with a second
// mate or end with a first one -- per batch a run of stride 2 over the pairs inside it, and a run of one pair when it ends
// between two mates.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

// A maximal stretch of pairs whose first mates lie in one batch and whose second mates lie in one batch: pair `pair` + j is
// read first_a + j * stride of batch ia and read first_b + j * stride of batch ib.  ia and ib index the per-file lists of
// non-empty batches: file 0's and file 1's, or, interleaved, the one list both.
struct PairRun { size_t ia, ib; uint64_t first_a, first_b, stride, n_pairs, pair; };

struct PairWalk {
    struct Range { size_t begin, end; };
    std::vector<PairRun> runs;        // in pair order
    std::vector<Range> touch[2];      // by file and batch: runs[begin, end) are the runs with a read of that batch (neighbours share a crossing run)
    int fb = 0;                       // the file side b's batches are of: 1 for two files, 0 interleaved

    // Every run of a paired input: n0, the read counts of file 0's non-empty batches; n1, file 1's, or null for an interleaved
    // input.  Null, or the refusal's line
    const char *build(const std::vector<uint64_t> &n0, const std::vector<uint64_t> *n1) {
        runs.clear();
        fb = n1 ? 1 : 0;
        touch[0].assign(n0.size(), Range{0, 0});
        touch[1].assign(n1 ? n1->size() : 0, Range{0, 0});
        uint64_t total[2] = {0, 0};
        for (const uint64_t n : n0) total[0] += n;
        if (n1) for (const uint64_t n : *n1) total[1] += n;
        if (n1 && total[0] != total[1]) return " Error: --in2: the files are not in step.";
        if (!n1 && (total[0] & 1)) return " Error: --interleaved: an odd number of reads.";
        auto add = [&](const PairRun &r) {
            for (Range *t : {&touch[0][r.ia], &touch[fb][r.ib]}) {
                if (!t->end) t->begin = runs.size();
                t->end = runs.size() + 1;
            }
            runs.push_back(r);
        };
        if (n1) {      // side by side: as many pairs a run as are left in the batch in hand of either file
            size_t ia = 0, ib = 0;
            uint64_t pa = 0, pb = 0, done = 0;
            while (ia < n0.size() && ib < n1->size()) {
                const uint64_t take = std::min(n0[ia] - pa, (*n1)[ib] - pb);
                add(PairRun{ia, ib, pa, pb, 1, take, done});
                done += take;
                if ((pa += take) == n0[ia]) { ++ia; pa = 0; }
                if ((pb += take) == (*n1)[ib]) { ++ib; pb = 0; }
            }
            return nullptr;
        }
        uint64_t at = 0;      // the ordinal of the batch's first record
        for (size_t i = 0; i < n0.size(); at += n0[i++]) {
            const uint64_t first = at & 1;      // (1: read 0 is the mate of the batch before's last read, in that batch's crossing run)
            const uint64_t inside = (n0[i] - first) / 2;
            if (inside) add(PairRun{i, i, first, first + 1, 2, inside, (at + first) / 2});
            // the last read's mate is the next batch's read 0 (there is one: the reads are even in number)
            if ((n0[i] - first) & 1) add(PairRun{i, i + 1, n0[i] - 1, 0, 1, 1, (at + n0[i] - 1) / 2});
        }
        return nullptr;
    }
};
