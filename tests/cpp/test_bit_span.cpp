// Stand-alone check of bow_amd/csrc/bit_span.h (no HIP, no library): the word view and the byte range of "n bits from bit `offset`
// of a byte buffer" against a bit-by-bit model over a host byte array.  Built with -fsanitize=address,undefined by
// tests/test_bit_span_cpu.py; prints the number of cases and exits 0, or says what failed and exits 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../bow_amd/csrc/bit_span.h"

using namespace bowgpu;

static int failures = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (failures++ < 20) {                           \
                printf("FAIL %s: ", #cond);                  \
                printf(__VA_ARGS__);                         \
                printf("\n");                                \
            }                                                \
        }                                                    \
    } while (0)

static int source_bit(const uint8_t *bytes, int64_t bit) { return (bytes[bit >> 3] >> (bit & 7)) & 1; }
// bit `bit` of the 32-bit words at `words` (little-endian words, as the kernels load them), read no further than words[nwords - 1]
static int word_bit(const uint8_t *words, int64_t nwords, int64_t bit) {
    if ((bit >> 5) >= nwords) return -1;
    uint32_t w;
    memcpy(&w, words + 4 * (bit >> 5), 4);
    return (w >> (bit & 31)) & 1;
}

int main() {
    const int64_t ns[] = {0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 200};
    // the caller's bytes inside an 8-byte aligned block, 8 bytes of slack in front for the misalignment
    alignas(8) static uint8_t block[8 + 64];
    uint32_t x = 12345;
    for (size_t i = 0; i < sizeof block; i++) { x = x * 1664525u + 1013904223u; block[i] = (uint8_t)(x >> 24); }
    long cases = 0;
    for (int mis = 0; mis < 8; mis++) {
        const uint8_t *bytes = block + mis;   // (offset + n <= 270 bits = 34 bytes: inside the block)
        for (int64_t offset = 0; offset <= 70; offset++) {
            for (int64_t n : ns) {
                cases++;
                // ---- read in place: the address rounded down to a word
                const BitWords w = bit_words(reinterpret_cast<uintptr_t>(bytes), offset, n);
                CHECK((w.addr & 3) == 0, "mis=%d", mis);
                CHECK(w.addr <= reinterpret_cast<uintptr_t>(bytes) && reinterpret_cast<uintptr_t>(bytes) - w.addr < 4, "mis=%d", mis);
                const uint8_t *words = reinterpret_cast<const uint8_t *>(w.addr);
                for (int64_t i = 0; i < n; i++)
                    CHECK(word_bit(words, w.words, w.bit0 + i) == source_bit(bytes, offset + i), "in place mis=%d offset=%lld n=%lld i=%lld", mis,
                          (long long)offset, (long long)n, (long long)i);
                if (n > 0) {
                    CHECK(w.words * 32 > w.bit0 + n - 1, "in place: the words do not cover the last row");
                    CHECK((w.words - 1) * 32 <= w.bit0 + n - 1, "in place: a word beyond the last row's");
                }
                // ---- staged: the bytes that hold the rows, in a zeroed block of the padded size
                const BitBytes b = bit_bytes(offset, n);
                CHECK(b.first == (offset >> 3) && (int64_t)b.count == ((offset + n + 7) >> 3) - (offset >> 3), "byte range offset=%lld n=%lld",
                      (long long)offset, (long long)n);
                CHECK(b.bit0 == (offset & 7), "bit0 offset=%lld", (long long)offset);
                const size_t padded = temp_bits_bytes(b.count);
                CHECK(padded % 4 == 0 && padded >= ((b.count + 3) & ~(size_t)3) + 16, "padded size of %zu bytes", b.count);
                std::vector<uint32_t> staged(padded / 4, 0u);   // (exactly `padded` bytes: the sanitizer sees a read beyond them)
                if (b.count) memcpy(staged.data(), bytes + b.first, b.count);
                const BitWords s = bit_words(reinterpret_cast<uintptr_t>(staged.data()), b.bit0, n);
                CHECK(s.addr == reinterpret_cast<uintptr_t>(staged.data()) && s.bit0 == b.bit0, "staged view");
                CHECK((size_t)s.words * 4 <= padded, "staged: %lld words beyond the padded size %zu", (long long)s.words, padded);
                for (int64_t i = 0; i < n; i++)
                    CHECK(word_bit(reinterpret_cast<const uint8_t *>(staged.data()), s.words, s.bit0 + i) == source_bit(bytes, offset + i),
                          "staged offset=%lld n=%lld i=%lld", (long long)offset, (long long)n, (long long)i);
                if (n > 0) CHECK(s.words * 32 > s.bit0 + n - 1, "staged: the words do not cover the last row");
            }
        }
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("cases %ld\n", cases);
    return 0;
}
