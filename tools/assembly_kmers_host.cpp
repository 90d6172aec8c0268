// The k-mer stage of phmm_assembly_kmers as a plain single-threaded host loop over the same arrays, std::unordered_set<std::string>
// for every set: what tools/assembly_kmers_bench.py times beside the device call, for scale (no gate).  It follows the reference's
// order -- per k and region: every run's scan from 0, then the start search and the positions threaded -- and returns the sizes of
// the non-unique set and of the vertex map, which the tool compares with the device's.
// Built by lorikeet_amd/csrc/Makefile into tools/libassembly_kmers_host.so.
#include <cstdint>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

namespace {

using Set = std::unordered_set<std::string>;

void scan(const uint8_t *seq, uint32_t stop, uint32_t k, Set &non_unique) {
    if (stop < k) return;
    Set all;
    for (uint32_t i = 0; i + k <= stop; ++i) {
        std::string kmer((const char *)seq + i, k);
        if (!all.insert(kmer).second) non_unique.insert(std::move(kmer));
    }
}

}  // namespace

extern "C" void assembly_kmers_host(uint32_t n_regions, const uint32_t *region_ref_off, const uint8_t *ref_bases, const uint32_t *region_read_off,
                                    const uint32_t *read_off, const uint8_t *read_bases, const uint8_t *read_quals, uint32_t n_k, const uint32_t *ks,
                                    uint32_t min_base_quality, uint32_t *n_non_unique, uint32_t *n_tracked) {
    for (uint32_t i = 0; i < n_k; ++i) {
        const uint32_t k = ks[i];
        for (uint32_t g = 0; g < n_regions; ++g) {
            const uint8_t *ref = ref_bases + region_ref_off[g];
            const uint32_t ref_len = region_ref_off[g + 1] - region_ref_off[g];
            uint32_t &nu = n_non_unique[i * n_regions + g], &tr = n_tracked[i * n_regions + g];
            nu = tr = 0;
            if (ref_len < k) continue;
            Set non_unique, tracked;
            std::vector<std::pair<uint32_t, std::pair<uint32_t, uint32_t>>> runs;   // read, [start, stop)
            scan(ref, ref_len, k, non_unique);
            for (uint32_t r = region_read_off[g]; r < region_read_off[g + 1]; ++r) {
                const uint8_t *b = read_bases + read_off[r], *q = read_quals + read_off[r];
                const uint32_t len = read_off[r + 1] - read_off[r];
                int64_t last_good = -1;
                for (uint32_t end = 0; end <= len; ++end) {
                    if (end == len || (b[end] & 0xdf) == 'N' || q[end] < min_base_quality) {
                        if (last_good >= 0 && end - last_good >= k) {
                            runs.push_back({r, {(uint32_t)last_good, end}});
                            scan(b, end, k, non_unique);
                        }
                        last_good = -1;
                    } else if (last_good < 0) {
                        last_good = end;
                    }
                }
            }
            const auto thread = [&](const uint8_t *seq, uint32_t from, uint32_t stop) {
                for (uint32_t p = from; p + k <= stop; ++p) {
                    std::string kmer((const char *)seq + p, k);
                    if (!non_unique.count(kmer)) tracked.insert(std::move(kmer));
                }
            };
            if (ref_len > k) thread(ref, 0, ref_len);
            for (const auto &run : runs) {
                const uint8_t *b = read_bases + read_off[run.first];
                const uint32_t start = run.second.first, stop = run.second.second;
                for (uint32_t p = start; p + k < stop; ++p)
                    if (!non_unique.count(std::string((const char *)b + p, k))) {
                        thread(b, p, stop);
                        break;
                    }
            }
            nu = (uint32_t)non_unique.size();
            tr = (uint32_t)tracked.size();
        }
    }
}
