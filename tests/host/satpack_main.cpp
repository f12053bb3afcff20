// satpack_main — which epilogue form the library picks for a fused INT8 chain (csrc/bn_chain_plan.cpp: tail2_plan sets Tail2Args::satpack
// from tail2_satpack_ok), on descriptor tables from a file, without the library, the C ABI or a device.  tests/test_satpack_forms.py
// builds it with the address and undefined-behaviour sanitizers.
//
//   satpack_main FORM N_LAYERS NC WORDS.bin [EDITS.bin]
//
// FORM: tail2 (i8_tail2_kernel) or mid (i8_mid2_kernel; also through its resident placement, which must carry the same choice).
// WORDS.bin: the descriptor tensor, raw little-endian int32.  Prints one line for the table as it is, then one line per (index, value) pair
// of EDITS.bin for the table with that single word replaced: -1 = the planner refuses the table, else Tail2Args::satpack (0 or 1).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "bn_chain_plan.h"

namespace {

std::vector<int32_t> read_words(const char* path) {
    std::vector<int32_t> words;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) return words;
    int32_t buf[256];
    for (size_t n; (n = std::fread(buf, sizeof buf[0], 256, f)) > 0;) words.insert(words.end(), buf, buf + n);
    std::fclose(f);
    return words;
}

int form_of(bool mid, int n_layers, int nc, const std::vector<int32_t>& words) {
    bn::Tail2Args a{};
    a.NC = nc;
    if (!bn::tail2_plan(words.data(), (int)words.size(), n_layers, a, mid)) return -1;
    if (a.satpack != (bn::tail2_satpack_ok(a) ? 1 : 0)) return -2;
    if (mid) {
        bn::Tail2Args r = a;
        if (bn::tail2_plan_resident(r) && r.satpack != a.satpack) return -3;
    }
    return a.satpack;
}

}  // namespace

int main(int argc, char** argv) {
    const std::string form = argc > 1 ? argv[1] : "";
    if ((argc != 5 && argc != 6) || (form != "tail2" && form != "mid")) {
        std::fprintf(stderr, "usage: satpack_main tail2|mid N_LAYERS NC WORDS.bin [EDITS.bin]\n");
        return 2;
    }
    const bool mid = form == "mid";
    const int n_layers = std::atoi(argv[2]), nc = std::atoi(argv[3]);
    const std::vector<int32_t> words = read_words(argv[4]);
    std::printf("%d\n", form_of(mid, n_layers, nc, words));
    if (argc == 6) {
        const std::vector<int32_t> edits = read_words(argv[5]);
        for (size_t k = 0; k + 1 < edits.size(); k += 2) {
            std::vector<int32_t> w(words);
            if (edits[k] < 0 || (size_t)edits[k] >= w.size()) return 2;
            w[(size_t)edits[k]] = edits[k + 1];
            std::printf("%d\n", form_of(mid, n_layers, nc, w));
        }
    }
    return 0;
}
