// mu_refusal (cmf.jl_amd/csrc/cmf_mu_install.h, free of HIP) asked whether the HALS rule may run, for every form, every setting of the
// older gates and both values of option "hals_mask": one line "form|gates|hals_mask <tab> code <tab> message" per cell
// (tests/test_masked_hals_cpu.py reads them).  Its own main, compiled with -fsanitize=address,undefined.
#include "cmf_mu_install.h"

#include <cstdio>

int main()
{
    struct Form { const char *name; int div; double beta; bool mask; };
    const Form forms[8] = {{"square", CMF_DIV_SQUARE, 0.0, false}, {"square+mask", CMF_DIV_SQUARE, 0.0, true}, {"kl", CMF_DIV_KL, 0.0, false}, {"kl+mask", CMF_DIV_KL, 0.0, true},
                           {"is", CMF_DIV_IS, 0.0, false}, {"is+mask", CMF_DIV_IS, 0.0, true}, {"beta(0.5)", CMF_DIV_BETA, 0.5, false}, {"beta(0.5)+mask", CMF_DIV_BETA, 0.5, true}};
    int cells = 0;
    for (const Form &fm : forms)
        for (int g = 0; g < 8; ++g)
            for (int hm = 0; hm < 2; ++hm) {
                MuFacts f{fm.div, fm.beta, fm.mask, (g >> 2) & 1, (g >> 1) & 1, g & 1, 0, false, false, true};
                if (f.hals_mask != 0) return 1; // (the last member: an aggregate that ends at have_data leaves the option off)
                f.hals_mask = hm;
                for (const char *rule : {"HALS", "PGD"}) {
                    std::string msg;
                    const int code = mu_refusal(f, MuAsk{MU_ASK_SQUARE_RULE, 0, 0.0, 0, rule}, &msg);
                    if ((code == CMF_OK) != msg.empty()) return 2; // a text exactly when refused
                    std::printf("%s|%s|%d%d%d|%d\t%d\t%s\n", rule, fm.name, f.kl_mask, f.pq_mask, f.is_div, hm, code, msg.c_str());
                    ++cells;
                }
            }
    std::fprintf(stderr, "ok %d cells\n", cells);
    return 0;
}
