// The decision of csrc/cmf_recentre.h driven by a stand-alone program (its own main), built under ASan and UBSan by
// tests/test_recentre_cpu.py:  recentre_shift_driver FILE  reads "K N L" and K*N*L doubles (C hex floats, Julia order: k fastest) from
// FILE and prints the K shifts of cmfrc::shifts, one per line; refused arguments print "refused".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "cmf_recentre.h"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long K = 0, N = 0, L = 0;
    if (fscanf(f, "%lld %lld %lld", &K, &N, &L) != 3) return 2;
    const bool sane = K > 0 && N > 0 && L > 0;
    std::vector<double> W((size_t)(sane ? K * N * L : 1)); // exactly the tensor: one element past it is an ASan error
    char tok[64];
    for (double &w : W) {
        if (!sane) break;
        if (fscanf(f, "%63s", tok) != 1) return 2;
        w = strtod(tok, nullptr);
    }
    fclose(f);
    std::vector<int32_t> s((size_t)(sane ? K : 1), -99);
    if (cmfrc::shifts(W.data(), K, N, L, s.data())) {
        printf("refused\n");
        return 0;
    }
    for (int32_t v : s) printf("%d\n", (int)v);
    return 0;
}
