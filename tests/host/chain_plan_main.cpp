// chain_plan_main — the LDS planners of the fused INT8 chains (csrc/bn_chain_plan.cpp) on a descriptor table from a file, without the
// library, the C ABI or a device.  tests/test_chain_plan_host.py builds it with the address and undefined-behaviour sanitizers.
//
//   chain_plan_main                                    -> kTailLayerWords kTailHeadWords kTail2LayerWords kTailG kMidG
//   chain_plan_main FORM N_LAYERS NC WORDS.bin         -> 0 (refused), or
//       1 lds_bytes const_words mean_off fcw_off bar_off resident, then every block's LDS offsets in the order of its struct
//       (tail: x y w dwc pwc lut zp; the others: x y dw pw zp), then for mid and mid-resident the words of tail2_plan_dump
//   chain_plan_main FORM N_LAYERS NC WORDS.bin sweep   -> for every word i of the table and v = INT32_MIN, -1, INT32_MAX a line
//       "i v" followed by that output for the table with word i = v (one process for the whole sweep)
//
// FORM: tail (i8_tail_kernel), tail2 (i8_tail2_kernel), mid (i8_mid2_kernel, staged), mid-resident (its resident placement).
// WORDS.bin: the descriptor tensor as the plan holds it, raw little-endian int32; its length is the n_words the planner is given.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bn_chain_plan.h"

namespace {

using namespace bn;

std::vector<long> plan_line(const std::string& form, int n_layers, int nc, const std::vector<int32_t>& words) {
    const int n_words = (int)words.size();
    std::vector<long> out;
    if (form == "tail") {
        Tail8Args a{};
        a.NC = nc;
        if (!tail_plan(words.data(), n_words, n_layers, a)) return {0};
        out = {1, a.lds_bytes, tail_const_words(a), a.mean_off, a.fcw_off, -1, 0};
        for (int i = 0; i < a.n_layers; ++i) {
            const Tail8Layer& L = a.L[i];
            out.insert(out.end(), {L.x_off, L.y_off, L.w_off, L.dwc_off, L.pwc_off, L.lut_off, L.zp_off});
        }
        return out;
    }
    const bool mid = form != "tail2";
    Tail2Args a{};
    a.NC = nc;
    if (!tail2_plan(words.data(), n_words, n_layers, a, mid) || (form == "mid-resident" && !tail2_plan_resident(a))) return {0};
    out = {1, a.lds_bytes, tail2_const_words(a, mid), a.mean_off, a.fcw_off, a.bar_off, a.resident};
    for (int i = 0; i < a.n_layers; ++i) {
        const Tail2Layer& L = a.L[i];
        out.insert(out.end(), {L.x_off, L.y_off, L.dw_off, L.pw_off, L.zp_off});
    }
    if (mid) {
        std::vector<int> dump(5 + 6 * a.n_layers);
        if (!tail2_plan_dump(a, dump.data(), (int)dump.size())) return {0};
        out.insert(out.end(), dump.begin(), dump.end());
    }
    return out;
}

void put(const std::vector<long>& v) {
    for (size_t i = 0; i < v.size(); ++i) std::printf(i ? " %ld" : "%ld", v[i]);
    std::printf("\n");
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 1) {
        put({kTailLayerWords, kTailHeadWords, kTail2LayerWords, kTailG, kMidG});
        return 0;
    }
    const std::string form = argc > 1 ? argv[1] : "";
    const bool sweep = argc == 6 && !std::strcmp(argv[5], "sweep");
    std::FILE* f = (argc == 5 || sweep) && (form == "tail" || form == "tail2" || form == "mid" || form == "mid-resident") ? std::fopen(argv[4], "rb") : nullptr;
    if (!f) {
        std::fprintf(stderr, "usage: chain_plan_main [tail|tail2|mid|mid-resident N_LAYERS NC WORDS.bin [sweep]]\n");
        return 2;
    }
    const int n_layers = std::atoi(argv[2]), nc = std::atoi(argv[3]);
    std::vector<int32_t> words;
    int32_t buf[256];
    for (size_t n; (n = std::fread(buf, sizeof buf[0], 256, f)) > 0;) words.insert(words.end(), buf, buf + n);
    std::fclose(f);
    if (!sweep) {
        put(plan_line(form, n_layers, nc, words));
        return 0;
    }
    for (size_t i = 0; i < words.size(); ++i)
        for (const int32_t v : {INT32_MIN, -1, INT32_MAX}) {
            std::vector<int32_t> w(words);   // (a fresh allocation of exactly the table's size: a read beyond it is reported)
            w[i] = v;
            std::printf("%zu %d ", i, v);
            put(plan_line(form, n_layers, nc, w));
        }
    return 0;
}
