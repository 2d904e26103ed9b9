// The refusals of cmf.jl_amd/csrc/cmf_mu_install.h (free of HIP) at every cell of the walk of tests/mu_form_walk.py: one line
// "start|form|gates|request <tab> code <tab> message" per cell, for every gate setting (tests/test_mu_install_cpu.py looks up the ones the
// golden file holds).  Its own main, compiled with -fsanitize=address,undefined.
#include "cmf_mu_install.h"

#include <cstdio>

struct Form { const char *name; int div; double beta; bool mask; };
struct Request { const char *name; MuAsk ask; };

int main()
{
    const Form forms[8] = {{"square", CMF_DIV_SQUARE, 0.0, false}, {"square+mask", CMF_DIV_SQUARE, 0.0, true}, {"kl", CMF_DIV_KL, 0.0, false}, {"kl+mask", CMF_DIV_KL, 0.0, true},
                           {"is", CMF_DIV_IS, 0.0, false}, {"is+mask", CMF_DIV_IS, 0.0, true}, {"beta(0.5)", CMF_DIV_BETA, 0.5, false}, {"beta(0.5)+mask", CMF_DIV_BETA, 0.5, true}};
    const Request requests[] = {
        {"set_mask", {MU_ASK_SET_MASK}}, {"clear_mask", {MU_ASK_CLEAR_MASK}},
        {"kind_square", {MU_ASK_SET_KIND, CMF_DIV_SQUARE}}, {"kind_kl", {MU_ASK_SET_KIND, CMF_DIV_KL}}, {"kind_is", {MU_ASK_SET_KIND, CMF_DIV_IS}},
        {"beta_0.5", {MU_ASK_SET_BETA, 0, 0.5}}, {"beta_1.5", {MU_ASK_SET_BETA, 0, 1.5}}, {"beta_1.0", {MU_ASK_SET_BETA, 0, 1.0}}, {"beta_0.005", {MU_ASK_SET_BETA, 0, 0.005}},
        {"gram_1", {MU_ASK_SET_GRAM, 0, 0.0, 1}},
        {"kl_mask_0", {MU_ASK_GATE_OFF, 0, 0.0, 0, "kl_mask"}}, {"pq_mask_0", {MU_ASK_GATE_OFF, 0, 0.0, 0, "pq_mask"}}, {"is_div_0", {MU_ASK_GATE_OFF, 0, 0.0, 0, "is_div"}},
        {"pgd_set_mask", {MU_ASK_CLEAR_MASK, 0, 0.0, 1}},
        {"hals_update_motifs", {MU_ASK_SQUARE_RULE, 0, 0.0, 0, "HALS"}}, {"pgd_update_motifs", {MU_ASK_SQUARE_RULE, 0, 0.0, 0, "PGD"}},
        {"xortho_1_0_0", {MU_ASK_SET_XORTHO}},
    };
    const char *const starts[3] = {"plain", "gram", "xortho"};
    int cells = 0;
    for (int s = 0; s < 3; ++s)
        for (const Form &fm : forms) {
            if (s && fm.div + fm.mask) continue; // (gram = 1 and the weights exist beside the plain square form only)
            for (int g = 0; g < 8; ++g) {
                const MuFacts f{fm.div, fm.beta, fm.mask, (g >> 2) & 1, (g >> 1) & 1, g & 1, s == 1 ? 1 : 0, s == 2, false, true};
                for (const Request &r : requests) {
                    std::string msg;
                    const int code = mu_refusal(f, r.ask, &msg);
                    if ((code == CMF_OK) != msg.empty()) return 1; // a text exactly when refused
                    std::printf("%s|%s|%d%d%d|%s\t%d\t%s\n", starts[s], fm.name, f.kl_mask, f.pq_mask, f.is_div, r.name, code, msg.c_str());
                    ++cells;
                }
            }
        }
    // a group handle and one without data: refused whatever else holds, the group first; a request that does not exist
    std::string msg;
    MuFacts f{CMF_DIV_SQUARE, 0.0, false, 1, 1, 1, 0, false, true, false};
    for (int what : {MU_ASK_SET_MASK, MU_ASK_CLEAR_MASK, MU_ASK_SET_KIND, MU_ASK_SET_BETA})
        if (mu_refusal(f, MuAsk{what, CMF_DIV_KL, 0.5}, &msg) != CMF_ERR_UNSUPPORTED || msg.find("T-sharded groups") == std::string::npos) return 2;
    if (mu_refusal(f, MuAsk{MU_ASK_SET_BETA, 0, 1.0}, &msg) != CMF_ERR_ARG) return 3; // (beta's argument errors come before the group's)
    f.group = false;
    if (mu_refusal(f, MuAsk{MU_ASK_SET_MASK}, &msg) != CMF_ERR_STATE || mu_refusal(f, MuAsk{MU_ASK_SET_KIND, CMF_DIV_KL}, &msg) != CMF_ERR_STATE ||
        mu_refusal(f, MuAsk{MU_ASK_SET_KIND, CMF_DIV_SQUARE}, &msg) != CMF_OK || mu_refusal(f, MuAsk{MU_ASK_CLEAR_MASK, 0, 0.0, 1}, &msg) != CMF_OK)
        return 4;
    for (int kind : {-1, 3, 4})
        if (mu_refusal(f, MuAsk{MU_ASK_SET_KIND, kind}, &msg) != CMF_ERR_ARG) return 5;
    if (mu_refusal(f, MuAsk{99}, &msg) != CMF_ERR_ARG) return 6;
    std::fprintf(stderr, "ok %d cells\n", cells);
    return 0;
}
