// split3_host IN OUT -- csrc/device.h's split3_pair on the host (tests/test_split_operands_cpu.py).  IN: an even number of
// fp32 values.  OUT, per pair of values, six 32-bit words: h, m, l of the bf16x2 overload (bit-cast), then h, m, l of the
// packed-word overload; value a of a pair is the low half of each word.
#include <cstdio>
#include <vector>

#include "../scanobjectnn_amd/csrc/device.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    std::vector<float> x;
    for (float v[2]; fread(v, sizeof(float), 2, in) == 2;) x.insert(x.end(), v, v + 2);
    std::vector<unsigned> w;
    for (size_t i = 0; i < x.size(); i += 2) {
        bf16x2 h, m, l;
        unsigned wh, wm, wl;
        split3_pair(x[i], x[i + 1], h, m, l);
        split3_pair(x[i], x[i + 1], wh, wm, wl);
        w.insert(w.end(), {__builtin_bit_cast(unsigned, h), __builtin_bit_cast(unsigned, m), __builtin_bit_cast(unsigned, l), wh, wm, wl});
    }
    const bool ok = fwrite(w.data(), sizeof(unsigned), w.size(), out) == w.size();
    return (fclose(out) == 0 && ok) ? 0 : 4;
}
