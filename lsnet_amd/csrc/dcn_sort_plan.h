// Geometry and index arithmetic of the stable radix sort that builds the anchor lists of the deformable backward
// (dcn_gather_kernels.h: dcn_list_*_kernel), written once for the device kernels and, compiled by a host compiler, for the
// sequential emulation of tools/dcn_sort_emul.cpp (tests/test_dcn_sort_host.py runs it under the address and undefined-
// behaviour sanitizers against std::stable_sort).
//
// The samples of a launch are enumerated in ascending id s; a sample's key is the launch-wide id of its anchor, or the
// SENTINEL `nanchors` when it belongs to no list.  A stable sort by key leaves every list in ascending s and the sentinel
// samples behind all lists.  The sort is least-significant-digit first, two passes (three above 2^22 anchors) of equal
// digit width.  A pass cuts its input into blocks of DS_BLOCK consecutive elements: one workgroup of DS_WAVES waves, a wave
// owning DS_ROWS rows of 64 consecutive elements.  The position of an element in the pass's output is
//     [elements of all blocks with a smaller digit] + [elements with its digit in earlier blocks]      (scanned histogram)
//   + [elements with its digit in earlier waves of its block] + [... in earlier rows of its wave]       (LDS counts)
//   + [... in lower lanes of its row]                                                                    (ballots)
// -- every term counts elements that precede it in the input order, so equal digits keep that order.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if !defined(LSN_HD)
#if defined(__HIPCC__)
#define LSN_HD __host__ __device__ __forceinline__
#else
#define LSN_HD static inline
#endif
#endif

constexpr int DS_THREADS = 256;                      // workgroup
constexpr int DS_WAVES = DS_THREADS / 64;
constexpr int DS_ROWS = 8;                           // rows of 64 elements per wave
constexpr int DS_WAVE_KEYS = DS_ROWS * 64;           // 512
constexpr int DS_BLOCK = DS_WAVES * DS_WAVE_KEYS;    // 2048 elements per workgroup
constexpr int DS_KEY_THREADS = 1024;                 // workgroup of the keys / histogram kernels: DS_BLOCK / 1024 = 2 elements per thread
constexpr int DS_MAX_DIGIT_BITS = 11;                // LDS of the scatter: DS_WAVES + 1 arrays of 2^11 ints = 40 KB at most
constexpr int DS_MAX_DIGITS = 1 << DS_MAX_DIGIT_BITS;
static_assert((31 + 2) / 3 <= DS_MAX_DIGIT_BITS, "three passes cover the 31 bits of the largest key");

// bits of the largest key, the sentinel `nanchors` (nanchors >= 1)
LSN_HD int ds_key_bits(int nanchors)
{
    int b = 1;
    while (b < 31 && (nanchors >> b) != 0) ++b;
    return b;
}
LSN_HD int ds_passes(int nanchors) { return ds_key_bits(nanchors) <= 2 * DS_MAX_DIGIT_BITS ? 2 : 3; }
// digit width of every pass: <= DS_MAX_DIGIT_BITS for every int (a key has at most 31 bits: three passes of 11; the
// workspace plan of csrc/dcn_route.h admits fewer than 2^30 anchors -- three passes of 10 -- and checks the width it gets)
LSN_HD int ds_digit_bits(int nanchors)
{
    const int p = ds_passes(nanchors);
    return (ds_key_bits(nanchors) + p - 1) / p;
}
LSN_HD int ds_digit(int key, int pass, int digit_bits) { return (int)(((unsigned)key >> (pass * digit_bits)) & ((1u << digit_bits) - 1u)); }
LSN_HD int ds_blocks(int nsamples) { return (nsamples + DS_BLOCK - 1) / DS_BLOCK; }
// element of (block, wave, row, lane) in a pass's input order
LSN_HD int ds_elem(int block, int wave, int row, int lane) { return block * DS_BLOCK + wave * DS_WAVE_KEYS + row * 64 + lane; }
// histogram of a pass, digit-major: [digit][block], then the per-digit totals the row scan leaves behind it
LSN_HD size_t ds_hist_at(int digit, int block, int nblocks) { return (size_t)digit * nblocks + block; }
LSN_HD size_t ds_scatter_lds_bytes(int digit_bits) { return ((size_t)(DS_WAVES + 1) << digit_bits) * sizeof(int); }
LSN_HD size_t ds_hist_ints(int nsamples, int nanchors) { return ((size_t)ds_blocks(nsamples) + 1) << ds_digit_bits(nanchors); }
// output position: scanned base of (digit, block), the digit's count in earlier waves of the block, and inside the wave (in
// its earlier rows + in the lower lanes of the element's row)
LSN_HD int ds_position(int scanned_base, int earlier_waves, int in_wave) { return scanned_base + earlier_waves + in_wave; }
