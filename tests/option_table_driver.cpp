// The decisions of cmf.jl_amd/csrc/cmf_options.h (free of HIP) for the requests it reads from standard input, one per line:
// "kind <tab> name <tab> value", kind one of lone / group / short_group / shard (a lone handle; the front handle of a two-shard group of
// T = 300, L = 8; the same of T = 30, L = 8, too short for the Gram form; a per-process shard without a communicator).  Per request one
// line "kind|name|value <tab> code <tab> message <tab> target"; first the line "names <tab> <cmf_option_names>".  Returns 1 when two rows share a name or a refusal has no text.  Its own main, compiled with
// -fsanitize=address,undefined (tests/test_option_table_cpu.py).
#include "cmf_options.h"

#include <cstdio>
#include <cstdlib>

int main()
{
    for (const OptRow &a : kOptions)
        for (const OptRow &b : kOptions)
            if (&a != &b && std::strcmp(a.name, b.name) == 0) return 1;
    std::printf("names\t%s\n", opt_names().c_str());
    char line[512];
    int cells = 0;
    while (std::fgets(line, sizeof(line), stdin)) {
        char kind[32], name[128];
        int value = 0;
        if (std::sscanf(line, "%31[^\t]\t%127[^\t]\t%d", kind, name, &value) != 3) return 2;
        OptKind k{false, false, false, false};
        if (std::strcmp(kind, "group") == 0) k = OptKind{true, true, false, false, 300, 8, 2};
        else if (std::strcmp(kind, "short_group") == 0) k = OptKind{true, true, false, false, 30, 8, 2};
        else if (std::strcmp(kind, "shard") == 0) k = OptKind{false, false, true, true};
        else if (std::strcmp(kind, "lone") != 0) return 3;
        const OptDecision d = opt_decide(name, value, k, std::getenv("CMF_TEST_HOOKS") != nullptr);
        if ((d.rc == CMF_OK) != d.msg.empty() || (d.rc != CMF_OK && d.target != OPT_ON_NOTHING)) return 1;
        std::printf("%s|%s|%d\t%d\t%s\t%d\n", kind, name, value, d.rc, d.msg.c_str(), d.target);
        ++cells;
    }
    std::fprintf(stderr, "ok %d cells\n", cells);
    return 0;
}
