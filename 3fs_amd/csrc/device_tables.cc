// device_tables.cc -- the constant tables of crc_kernels.h, built on the host once per device
// context (O(tables) scalar GF(2) algebra, gf2.h).
#include "crc_kernels.h"
#include "internal.h"

namespace hf3fs_crc {
namespace {

void build_short_tables(ShortTables& T, uint32_t poly) {
  const uint32_t x32 = xpow_bits(32, poly), x8 = xpow_bits(8, poly);
  for (int k = 0; k < 4; ++k)
    for (uint32_t b = 0; b < 256; ++b) T.dw[k][b] = gf_mul(b << (8 * k), x32, poly);
  for (uint32_t b = 0; b < 256; ++b) T.b8[b] = gf_mul(b, x8, poly);
  for (int n = -kXs8Neg; n < kXs8Pos; ++n) T.xs8[kXs8Neg + n] = xpow_signed_bits(8ll * n, poly);
}

void build_fold_tables(FoldTables& T, uint32_t poly) {
  const uint32_t c0 = xpow_neg_bits(32, poly), ch = xpow_neg_bits(4096, poly);
  for (int j = 0; j < 8; ++j)
    for (uint32_t n = 0; n < 16; ++n) {
      const uint32_t a = n << (4 * j);
      for (int c = 0; c < 32; ++c) T.w[j][n][c] = gf_mul(a, xpow_neg_bits(128ull * c, poly), poly);
    }
  for (int k = 0; k < 4; ++k)
    for (uint32_t b = 0; b < 256; ++b) {
      T.c0[k][b] = gf_mul(b << (8 * k), c0, poly);
      T.ch[k][b] = gf_mul(b << (8 * k), ch, poly);
    }
}

void build_poly_tables(PolyTables& T, uint32_t poly) {
  const uint32_t k = xpow_bits(8ull * kBlockBytes, poly);
  for (int b = 0; b < 4; ++b)
    for (uint32_t i = 0; i < 256; ++i) T.step[b][i] = gf_mul(i << (8 * b), k, poly);
  T.xpow[0] = kOne >> 1;
  T.xinv[0] = x_inverse(poly);
  for (int i = 1; i < 64; ++i) {
    T.xpow[i] = gf_mul(T.xpow[i - 1], T.xpow[i - 1], poly);
    T.xinv[i] = gf_mul(T.xinv[i - 1], T.xinv[i - 1], poly);
  }
  for (int t = 0; t < kMulcTables; ++t) {
    const uint32_t c = xpow_neg_bits(t == 0 ? 32 : (128ull << (t - 1)), poly);
    for (int b = 0; b < 4; ++b)
      for (uint32_t i = 0; i < 256; ++i) T.mulc[t][b][i] = gf_mul(i << (8 * b), c, poly);
  }
  for (int p = 0; p < 16; ++p) T.xneg8[p] = xpow_neg_bits(8ull * p, poly);
  for (int p = 0; p < 16; ++p)
    for (int i = 0; i < 32; ++i) T.xneg8_cols[p][i] = gf_mul(T.xneg8[p], xpow_bits((uint64_t)i, poly), poly);
  for (int p = 0; p < 4; ++p) T.xpos8[p] = xpow_bits(8ull * p, poly);

  for (int j = 0; j < kPowDigits; ++j) {  // pow8b[j][d] = (x^(8 * 256^j))^d
    const uint32_t base = xpow_bits(8ull << (8 * j), poly), ibase = xpow_neg_bits(8ull << (8 * j), poly);
    T.pow8b[j][0] = T.inv8b[j][0] = kOne;
    for (int d = 1; d < 256; ++d) {
      T.pow8b[j][d] = gf_mul(T.pow8b[j][d - 1], base, poly);
      T.inv8b[j][d] = gf_mul(T.inv8b[j][d - 1], ibase, poly);
    }
  }
}

}  // namespace

void build_device_tables(DeviceTables& T) {
  const uint32_t polys[2] = {kPolyCrc32c, kPolyCrc32};
  for (int k = 0; k < 2; ++k) {
    build_poly_tables(T.poly[k], polys[k]);
    build_short_tables(T.sh[k], polys[k]);
    build_fold_tables(T.fold[k], polys[k]);
  }
}

}  // namespace hf3fs_crc
