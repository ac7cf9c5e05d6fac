// bit_span.h — the arithmetic of "n bits from bit `offset` of a caller's byte buffer" as the kernels read them: an aligned 32-bit
// word pointer and the bit index of row 0.  Pure: no HIP, no library state (tests/cpp/test_bit_span.cpp checks it against a
// bit-by-bit model); dev_cols.cpp does the aliasing, mapping and uploading around it.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace bowgpu {

// The one size rule of a bitmap on the device that the library allocates - a staged input, an output's working copy, a column of
// a temporary frame: its bytes rounded up to whole 32-bit words + 16.  The kernels that fill a frame store whole 32- or 64-bit
// validity words, and a 64-bit word may begin at the last 32-bit word of the rows and be followed by a reader's look at the word
// behind it.
inline size_t temp_bits_bytes(size_t bitmap_bytes) { return ((bitmap_bytes + 3) & ~(size_t)3) + 16; }

// Bits read where they lie (device memory, registered host memory, a staged block): the buffer's address rounded down to a word.
// Row i is bit `bit0 + i` counted from `addr`; `words` 32-bit words from there hold the n rows.
struct BitWords {
    uintptr_t addr;
    int64_t bit0, words;
};
inline BitWords bit_words(uintptr_t bytes_addr, int64_t offset, int64_t n) {
    const int64_t bit0 = (int64_t)(bytes_addr & 3) * 8 + offset;
    return {bytes_addr & ~(uintptr_t)3, bit0, (bit0 + n + 31) >> 5};
}

// Bits that have to be copied first: the bytes [first, first + count) of the buffer hold them, and in a word-aligned copy of
// exactly those bytes row 0 is bit `bit0` (= what bit_words gives for the copy and offset & 7).
struct BitBytes {
    int64_t first;
    size_t count;
    int64_t bit0;
};
inline BitBytes bit_bytes(int64_t offset, int64_t n) {
    const int64_t b0 = offset >> 3, b1 = (offset + n + 7) >> 3;
    return {b0, (size_t)(b1 - b0), offset & 7};
}

}  // namespace bowgpu
