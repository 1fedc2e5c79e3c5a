// matrix_encrypt.hip -- MI355X (gfx950), family 4: encryptBits (index.js:87-110) for a batch under ONE shared key as batch x Toeplitz
// matrix products on the int8 matrix cores (v_mfma_i32_32x32x32_i8, int32 accumulation: exact), the closed-form split by 1 - x^N
// (index.js:358-401) and the plaintext add (index.js:235-244) fused into the epilogue.  matrix_common.h holds the
// tile geometry and the strip loop; tools/mfma_model.py is the executable specification.
#include "matrix_encrypt_body.h"

__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_encrypt_m(MGeom g, u32 q, const u16 *__restrict__ h,
                                                             const uint8_t *__restrict__ r,
                                                             const uint8_t *__restrict__ m, long B,
                                                             u16 *__restrict__ e, u16 *__restrict__ quotE) {
  encrypt_m_body<4, false>(g, q, h, r, m, B, e, quotE);
}

__global__ __launch_bounds__(BLOCK_THREADS, 2) void k_encrypt_md(MGeom g, u32 q, const u16 *__restrict__ h,
                                                              const uint8_t *__restrict__ r,
                                                              const uint8_t *__restrict__ m, long B,
                                                              u16 *__restrict__ e, u16 *__restrict__ quotE) {
  encrypt_m_body<4, true>(g, q, h, r, m, B, e, quotE);
}

NTRU_STAMPS_READER(ntru_debug_read_stamps_enc)

// ---- host side ----------------------------------------------------------------------------------------------------------
// Kernel paths (ntru_engine_set_kernel_path): 0 = auto and 5 -> k_encrypt_md where a row fits one direct-to-LDS instruction, else
// k_encrypt_m; 4 -> k_encrypt_m.
int ntru_launch_encrypt_matrix(ntru_engine *eng, int N, int q, int ld, const uint16_t *d_h, const uint8_t *d_r, const uint8_t *d_m,
                               int64_t B, uint16_t *d_e, uint16_t *d_quotE) {
  MGeom mg;
  if (!make_mgeom(eng, N, q, ld, &mg)) return NTRU_NOT_TAKEN;
  const size_t lds = (size_t)32 * mg.tpitch + (size_t)32 * mg.pitchA + (((size_t)32 * ld + 15) & ~(size_t)15) + 16;
  const long nrb = (long)((B + 31) / 32);
  if (lds > 160 * 1024) return NTRU_NOT_TAKEN;
  // The default: the operands reach LDS by direct-to-LDS loads, r of the next row block ahead of the last epilogue's stores:
  // 1.49-1.51 ms against 1.57-1.62 ms per 2^20 at N = 821 on the same device (profiles/archive/r02_ab_direct_to_lds_rows.txt).
  // One direct-to-LDS instruction moves 64 x 16 bytes from the dword at or below a row, and eight of them per thread the m
  // image: a row of (its byte phase) + N > 1024 bytes, or an image of (phase) + 32 ld > 32768 bytes, would lose its last 1-3
  // bytes.  Those shapes (N >= 1022, or ld = 1024, with rows that are not dword-aligned) take k_encrypt_m, whose register
  // staging fetches the extra dword.
  const bool rows_dword_aligned = (ld & 3) == 0 && ((uintptr_t)d_r & 3) == 0, img_dword_aligned = (ld & 3) == 0 && ((uintptr_t)d_m & 3) == 0;
  const bool dma_fits = (N + 3 <= 1024 || (rows_dword_aligned && N <= 1024)) && (32 * ld + 3 <= 32768 || (img_dword_aligned && 32 * ld <= 32768));
  const bool md = eng->path != 4 && dma_fits;
  note_kernel(eng, md ? "k_encrypt_md" : "k_encrypt_m");
  return launch_resident(eng, md ? k_encrypt_md : k_encrypt_m, nrb, BLOCK_THREADS, lds, mg, (u32)q, d_h, d_r, d_m, (long)B, d_e, d_quotE);
}
