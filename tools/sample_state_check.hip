// The sampling passes on final states that are written down, not simulated: a case file describes populations by their
// summaries {n-, n+}, bin counters and rows, and this program hands them to the library's own compiled passes
// (launch_subsample, launch_passage, launch_keep: build/ssa_subsample.o and build/ssa_passage.o, linked in; no kernel is
// defined here) and writes back what they produce. 256 u32 counters describe billions of N+ cells, so subsample mapping
// v1 (include/ecdna_ssa.h) runs at population sizes up to 2^32 that no stepper reaches within a test:
// Lemire rejection, further Philox blocks per draw, positions above 2^31, prefix sums near 2^32 and the guards.
// Verification tool (tests/test_gpu_sample_states.py compares with tests/subsample_law.py).
// Build: ecdna-evo_amd/Makefile (bin/sample_state_check; __graft_entry__.build() runs it)
//
// Usage: sample_state_check CASES RESULTS. Both files are little-endian arrays as numpy writes them.
// CASES:   u64 magic, u64 count, then per case
//   u64 head[kHead]: pass (0 subsample, 1 passage with founders, 2 passage without: the last phase, 3 keep), n, bag_k,
//     counter bytes (0 none, 2, 4), row_stride, row_pad, bins, m, table_slots (0: subsample_table_slots(m), as
//     ssa_api.cpp; else the case overrides it), sort_slots (0: passage_sort_slots(m)), seed, rid0, rid_stride,
//     reps_per_set, reps_per_block, has_target, n_sets, founder_stride
//   u64 nminus[n], u64 nplus[n], counters[n][bag_k] (u16 / u32), u16 rows[n * row_stride + row_pad],
//   u64 target[bins] if has_target
// RESULTS: u64 magic, u64 count, then per case
//   stats[n] (ecdna_rep_stats_t), u64 sample_hist[n_sets][bins], u32 founder_counts[n][2], u16 founder_rows[n][stride]
// Every device buffer has the size the case declares (rows: n * row_stride + row_pad cells, whatever the summaries
// claim); before a launch, stats and founders are filled with 0xEE bytes and the histogram with zeros, so what a pass
// leaves alone shows. One stream; the first HIP error ends the program with nothing more launched.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "ssa_launch.h"

namespace {

constexpr uint64_t kMagic = 0x4b43485353ull;  // "SSHCK"
constexpr int kHead = 18;
constexpr uint8_t kFill = 0xEE;

#define HIP_OK(expr)                                                                               \
    do {                                                                                           \
        const hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                                    \
            fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return 3;                                                                              \
        }                                                                                          \
    } while (0)

template <typename T>
bool read_n(FILE* f, std::vector<T>& v, uint64_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
bool write_n(FILE* f, const std::vector<T>& v) {
    return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int bad_case(uint64_t i, const char* what) {
    fprintf(stderr, "case %llu: %s\n", (unsigned long long)i, what);
    return 2;
}

// A device buffer of the host vector's size and contents.
template <typename T>
hipError_t upload(T** d, const std::vector<T>& h) {
    *d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), (h.size() ? h.size() : 1) * sizeof(T));
    if (e == hipSuccess && !h.empty()) e = hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}
template <typename T>
hipError_t filled(T** d, uint64_t count, int byte) {
    *d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(d), (count ? count : 1) * sizeof(T));
    if (e == hipSuccess) e = hipMemset(*d, byte, (count ? count : 1) * sizeof(T));
    return e;
}
template <typename T>
hipError_t download(std::vector<T>& h, const T* d, uint64_t count) {
    h.resize(count);
    return count ? hipMemcpy(h.data(), d, count * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
}

// The target's CDF over the bins and its mean / entropy / N+ frequency, as the host computes them when a context is
// created (ssa_api.cpp, summarize_targets).
void summarize_target(const std::vector<uint64_t>& hist, std::vector<double>& cdf, double sc[3]) {
    const size_t bins = hist.size();
    double tot = 0.0;
    for (size_t b = 0; b < bins; ++b) tot += (double)hist[b];
    double acc = 0.0, ksum = 0.0, ent = 0.0;
    cdf.resize(bins);
    for (size_t b = 0; b < bins; ++b) {
        const double pb = (double)hist[b] / tot;
        acc += pb;
        cdf[b] = acc;
        ksum += (double)b * (double)hist[b];
        if (pb > 0.0) ent -= pb * log(pb);
    }
    sc[0] = ksum / tot;
    sc[1] = ent;
    sc[2] = 1.0 - (double)hist[0] / tot;
}

int run_case(uint64_t ci, FILE* in, FILE* out, hipStream_t st) {
    std::vector<uint64_t> h;
    if (!read_n(in, h, kHead)) return bad_case(ci, "short header");
    const uint64_t pass = h[0], n = h[1], bag_k = h[2], cbytes = h[3], row_stride = h[4], row_pad = h[5], bins = h[6],
                   m = h[7], seed = h[10], rid0 = h[11], rid_stride = h[12], reps_per_set = h[13],
                   reps_per_block = h[14], has_target = h[15], n_sets = h[16];
    // what the launchers and kernels take for granted of their host (ssa_api.cpp's validation and planner)
    if (pass > 3 || n < 1 || n > 4096) return bad_case(ci, "pass or n");
    if (!((bag_k == 0 && cbytes == 0) || ((bag_k == 32 || bag_k == 64 || bag_k == 256) && (cbytes == 2 || cbytes == 4))))
        return bad_case(ci, "bag_k / counter bytes");
    if (row_stride < 64 || row_stride % 64 || row_stride > (1u << 22) || row_pad > (1u << 22))
        return bad_case(ci, "row_stride must be a multiple of 64");
    if (bins < 2 || bins > 2048 || m < 1 || m > ecdna::kMaxSubsampleCells) return bad_case(ci, "bins or m");
    if (rid_stride < 1 || reps_per_set < 1 || reps_per_block < 1 || reps_per_block > n || n_sets < 1 || n_sets > 64)
        return bad_case(ci, "ids");
    if (rid0 > ~0ull - (n - 1) * rid_stride || (rid0 + (n - 1) * rid_stride) / reps_per_set >= n_sets)
        return bad_case(ci, "replicate ids map past n_sets");
    const uint64_t table_slots = h[8] ? h[8] : ecdna::subsample_table_slots((uint32_t)m);
    const uint64_t sort_slots = h[9] ? h[9] : ecdna::passage_sort_slots((uint32_t)m);
    const uint64_t founder_stride = h[17] ? h[17] : (pass == 3 ? m : (m + 63) / 64 * 64);
    if (table_slots > 2 * 4096 || sort_slots > 4096 || founder_stride < m || founder_stride > 8192)
        return bad_case(ci, "slots or founder_stride");

    std::vector<uint64_t> nminus, nplus, target;
    std::vector<uint8_t> counters;
    std::vector<uint16_t> rows;
    if (!read_n(in, nminus, n) || !read_n(in, nplus, n) || !read_n(in, counters, n * bag_k * cbytes) ||
        !read_n(in, rows, n * row_stride + row_pad) || !read_n(in, target, has_target ? bins : 0))
        return bad_case(ci, "short arrays");
    std::vector<ecdna_rep_summary_t> summaries(n);
    for (uint64_t q = 0; q < n; ++q) {
        memset(&summaries[q], 0, sizeof(ecdna_rep_summary_t));
        summaries[q].nminus = nminus[q];
        summaries[q].nplus = nplus[q];
    }

    ecdna_rep_summary_t* d_sum;
    uint8_t* d_bags;
    uint16_t *d_rows, *d_frows;
    ecdna_rep_stats_t* d_stats;
    uint64_t* d_hist;
    uint2* d_fcounts;
    double* d_cdf = nullptr;
    HIP_OK(upload(&d_sum, summaries));
    HIP_OK(upload(&d_bags, counters));
    HIP_OK(upload(&d_rows, rows));
    HIP_OK(filled(&d_stats, n, kFill));
    HIP_OK(filled(&d_hist, n_sets * bins, 0));
    HIP_OK(filled(&d_fcounts, n, kFill));
    HIP_OK(filled(&d_frows, n * founder_stride, kFill));
    ecdna::StatsTarget tgt{};
    if (has_target) {
        double tot = 0.0;
        for (uint64_t v : target) tot += (double)v;
        if (!(tot > 0.0)) return bad_case(ci, "empty target");
        std::vector<double> cdf;
        double sc[3];
        summarize_target(target, cdf, sc);
        HIP_OK(upload(&d_cdf, cdf));
        tgt = ecdna::StatsTarget{d_cdf, sc[0], sc[1], sc[2], 1u};
    }

    const ecdna::FinalState fs{d_rows, d_sum, row_stride, bag_k ? d_bags : nullptr, (uint32_t)bag_k, cbytes == 4 ? 1u : 0u};
    const ecdna::ChunkIds ids{rid0, rid_stride, reps_per_set, (uint32_t)n, (uint32_t)bins, (uint32_t)reps_per_block};
    const uint32_t blocks = (uint32_t)((n + reps_per_block - 1) / reps_per_block);
    if (pass == 0) {
        ecdna::SubsampleArgs sa{};
        sa.state = fs;
        sa.ids = ids;
        sa.target = tgt;
        sa.stats = d_stats;
        sa.sample_hist = d_hist;
        sa.seed = seed;
        sa.m = (uint32_t)m;
        sa.table_slots = (uint32_t)table_slots;
        HIP_OK(ecdna::launch_subsample(sa, blocks, st));
    } else {
        ecdna::PassageArgs pa{};
        pa.state = fs;
        pa.ids = ids;
        pa.seed = seed;
        pa.m = (uint32_t)m;
        pa.table_slots = (uint32_t)table_slots;
        pa.sort_slots = (uint32_t)sort_slots;
        pa.founder_counts = d_fcounts;
        pa.founder_stride = founder_stride;
        if (pass == 3) {  // (the keep pass reads neither stats, sample_hist nor target: ssa_api.cpp leaves them null)
            pa.founder_rows = d_frows;
            HIP_OK(ecdna::launch_keep(pa, blocks, st));
        } else {
            pa.target = tgt;
            pa.stats = d_stats;
            pa.sample_hist = d_hist;
            pa.founder_rows = pass == 1 ? d_frows : nullptr;
            HIP_OK(ecdna::launch_passage(pa, blocks, st));
        }
    }
    HIP_OK(hipStreamSynchronize(st));
    HIP_OK(hipGetLastError());

    std::vector<ecdna_rep_stats_t> o_stats;
    std::vector<uint64_t> o_hist;
    std::vector<uint2> o_fcounts;
    std::vector<uint16_t> o_frows;
    HIP_OK(download(o_stats, d_stats, n));
    HIP_OK(download(o_hist, d_hist, n_sets * bins));
    HIP_OK(download(o_fcounts, d_fcounts, n));
    HIP_OK(download(o_frows, d_frows, n * founder_stride));
    for (void* p : {(void*)d_sum, (void*)d_bags, (void*)d_rows, (void*)d_stats, (void*)d_hist, (void*)d_fcounts,
                    (void*)d_frows, (void*)d_cdf})
        if (p) HIP_OK(hipFree(p));
    if (!write_n(out, o_stats) || !write_n(out, o_hist) || !write_n(out, o_fcounts) || !write_n(out, o_frows)) {
        fprintf(stderr, "case %llu: cannot write results\n", (unsigned long long)ci);
        return 2;
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    static_assert(sizeof(ecdna_rep_stats_t) == 64 && sizeof(uint2) == 8, "record sizes of the result file");
    if (argc != 3) {
        fprintf(stderr, "usage: %s CASES RESULTS\n", argv[0]);
        return 2;
    }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = in ? fopen(argv[2], "wb") : nullptr;
    uint64_t top[2] = {0, 0};
    if (!in || !out || fread(top, 8, 2, in) != 2 || top[0] != kMagic || top[1] > 4096 || fwrite(top, 8, 2, out) != 2) {
        fprintf(stderr, "cannot open the files, or no case file\n");
        return 2;
    }
    hipStream_t st;
    HIP_OK(hipStreamCreate(&st));
    for (uint64_t ci = 0; ci < top[1]; ++ci) {
        const int rc = run_case(ci, in, out, st);
        if (rc) return rc;
    }
    HIP_OK(hipStreamDestroy(st));
    if (fclose(out) != 0) return 2;
    fclose(in);
    printf("{\"cases\": %llu}\n", (unsigned long long)top[1]);
    return 0;
}
