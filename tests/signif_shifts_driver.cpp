// The HIP-free part of csrc/cmf_signif.h driven by a stand-alone program (its own main), built under ASan and UBSan by
// tests/test_significance_cpu.py:  signif_shifts_driver seed first_draw n_draws K N L  prints the table of cmf_null_shifts, one value
// per line, (n fastest, then k, then the draw); refused arguments print "refused".  Also prints default_batch(K) as the last line.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cmf_signif.h"

int main(int argc, char **argv)
{
    if (argc != 7) return 2;
    const uint64_t seed = strtoull(argv[1], nullptr, 10);
    const int64_t first = atoll(argv[2]), n = atoll(argv[3]), K = atoll(argv[4]), N = atoll(argv[5]), L = atoll(argv[6]);
    std::vector<int32_t> s((size_t)(n > 0 && K > 0 && N > 0 ? n * K * N : 1), -1); // exactly the table: one element past it is an ASan error
    if (cmfsig::null_shifts(seed, first, n, K, N, L, s.data())) {
        printf("refused\n");
        return 0;
    }
    for (int32_t v : s) printf("%d\n", (int)v);
    printf("batch %lld\n", (long long)cmfsig::default_batch(K));
    return 0;
}
