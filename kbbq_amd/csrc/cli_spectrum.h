// cli_spectrum.h -- --estimate-genomelen and --spectrum FILE: the k-mer spectrum of the reads, counted on the GPU between the
// first scan and derive_sampling (kbbq_engine.h: kbbq_spectrum_*), and the genome length it gives where the run would
// otherwise stop for lack of one.  Compiled into kbbq_cli.cc alone, behind PassBatches.
#pragma once

// The spectrum of every batch of `reads` -- the resident device batches, or the host parsers reading the file once more --
// on device 0, in a table of 2^KBBQ_SPECTRUM_SLOTS_LOG2 slots that is freed again before the engine and its filters exist;
// the sample is sized by the bases the scan counted, so the table never passes half full.  --spectrum: the file.
// need_length: the run has no other genome length; *genomelen gets the estimate, and a spectrum without a coverage peak ends
// the run.  Returns 0, or the exit status with the message on stderr.
static int count_spectrum(const CliOptions &o, const ScanState &s, const PassBatches &reads, bool need_length, uint64_t *genomelen) {
    std::cerr << put_now << " Estimating genome length from the k-mer spectrum." << std::endl;
    uint32_t shift = 0;
    if (kbbq_host_spectrum_shift(s.seqlen, (uint32_t)o.spectrum_slots_log2, &shift) < 0) return fail_engine("KBBQ_SPECTRUM_SLOTS_LOG2");
    struct Handle {
        kbbq_spectrum *h = nullptr;
        ~Handle() { if (h) kbbq_spectrum_destroy(h); }
    } spec;
    // (no smaller table on a failure: the sample, and with it the estimate, would depend on the memory that happens to be free)
    if (kbbq_spectrum_create(0, o.k, (uint32_t)o.spectrum_slots_log2, shift, &spec.h) < 0) return fail_engine("cannot create the k-mer spectrum table");
    if (!reads.each(true, [&](const kbbq_reads &b, size_t) { return kbbq_spectrum_batch(spec.h, &b) >= 0; })) return fail_engine("counting k-mers");
    if (reads.fatal()) return 1;
    kbbq_spectrum_result res;
    if (kbbq_spectrum_finish(spec.h, &res) < 0) return fail_engine("counting k-mers");
    kbbq_spectrum_destroy(spec.h);      // the table goes back before the filters are allocated
    spec.h = nullptr;
    kbbq_spectrum_estimate est;
    const int none = kbbq_host_spectrum_estimate(&res, &est);
    if (none < 0) return fail_engine("estimating the genome length");
    char coverage[32];
    snprintf(coverage, sizeof coverage, "%llu.%03llu", (unsigned long long)(est.kmer_coverage_milli / 1000), (unsigned long long)(est.kmer_coverage_milli % 1000));
    std::cerr << put_now << " Counted " << res.valid_positions << " valid kmers, 1 in 2^" << shift << " of the distinct ones: " << res.distinct
              << " distinct, valley at " << est.valley << ", peak at " << est.peak << ", kmer coverage " << coverage << "." << std::endl;
    if (!o.spectrum.empty() && kbbq_host_spectrum_write(o.spectrum.c_str(), &res, &est) < 0) return fail_engine("writing the k-mer spectrum");
    if (!need_length) return 0;
    if (none)
        return give_up(" Error: the k-mer spectrum of " + o.filename + " shows no coverage peak (coverage too low, or too few reads);"
                       " please provide the genome length on the command line using the --genomelen option.");
    std::cerr << put_now << " Genome length is " << est.genome_length << " bp." << std::endl;
    *genomelen = est.genome_length;
    return 0;
}
