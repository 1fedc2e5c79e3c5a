"""Every kernel instantiation the library compiles, with a call that launches it.

Plain data, imported by tests/test_build_quality.py (every compiled instantiation has a row and every row names one), by
tests/test_kernel_variants_gpu.py (each row's calls against the oracle, through the runners of tests/variant_runners.py, and the
dispatch sweep) and by tests/valu_geometry.py (the K ranges; the rows pin its restatement of the launchers).  Not a test module.

A row:
  kernel  the demangled instantiation as `c++filt` prints it, return type and argument list dropped ("k_decrypt_s<11, 11, true>")
  entry   the C-ABI entry point whose launcher selects it (the name without the ntru_ prefix and the _batch[_dev] suffix)
  shapes  calls that select it: dicts of N, q, p, path (ntru_engine_set_kernel_path), B and extra.  The first has the smallest N that
          selects the kernel; a second, larger N follows where the selection rule spans a wide range.  For the entry points
          without a scheme modulus, q is the modulus (add, split_by_I, polymul_split, sum_groups: `mod`), the largest value (pack,
          pack_bytes, unpack), 2^20 (generic_multiply) or 0 (bytes_to_rows, rows_to_bytes); p is the sampler's rounds
          (sample_ternary) and 0 elsewhere.  `extra` holds what else the call takes (empty for most entries):
            sum_groups                    B = the number of rows; K = rows per uniform group, or csr = True for the offsets form
                                          (empty groups first, last and in the middle); weights = True / False where the row fixes it
            bytes_to_rows, rows_to_bytes  nbytes = message bytes per row (1 <= nbytes <= N / 8)
            check_*                       q, p are the circuit's moduli, the bit counts are calculateNq / calculateNp of them (at N = 2
                                          they accept an honest VerifyDecrypt witness only for q <= 47: q = 32); B = the accepted
                                          witnesses of a call (the mutated ones come on top)
            keygen                        df, dg of a parameter set whose first draws hold non-units, and first = a first_item at which
                                          the B items from first, first - 1 and first - 2 on hold one (item 316 at N = 17)
            sum_groups_packed             layout = the lane layout N gives the row's field width (packed_layout below): "side" (U <= 32,
                                          several rows side by side in a wave), "row" (32 < U <= 64) or "tiles" (U > 64); weights as
                                          for sum_groups.  The group layouts and the row counts are the runner's (B is not used): the
                                          large launch takes its row count from the device's CU count
            decrypt_packed                q is the scheme's modulus: one shape per field width, N with a field across a 64-bit limb
                                          (where the width allows one) and a partial last element
  last    what ntru_engine_last_kernel() returns after the call
  rule    where the launcher writes a coarse name or none: the selection rule the shapes satisfy (nw = (N + 32) / 32 etc.)
  unreachable  set instead of shapes when no call the ABI accepts selects the instantiation, with the reason
  addend_one_only  on a row of the decrypt family (LIFT_ENTRIES) whose selection rule admits no shape at which the centred lift's addend
               (p - q % p) % p differs from 1, the reason; None on every other row.  The runners decrypt in both lift modes, and only at
               such a shape do the modes give different values
"""
import math

import numpy as np

ROWS = []


def _row(kernel, entry, shapes, last=None, rule=None, unreachable=None):
    ROWS.append({"kernel": kernel, "entry": entry,
                 "shapes": [dict(N=t[0], q=t[1], p=t[2], path=t[3], B=t[4], extra=dict(t[5]) if len(t) > 5 else {}) for t in shapes],
                 "last": last, "rule": rule, "unreachable": unreachable, "addend_one_only": None})


# K of the vector-ALU families: the smallest odd K with ceil(N / 2K) <= 64
K_RANGES = {1: (2, 128), 3: (129, 384), 5: (385, 640), 7: (641, 896), 9: (897, 1152), 11: (1153, 1408), 13: (1409, 1664),
            15: (1665, 1920)}

# ---- encrypt -------------------------------------------------------------------------------------------------------------------
_row("k_encrypt_md", "encrypt", [(64, 2048, 0, 0, 33), (821, 4096, 0, 0, 95)], "k_encrypt_md")
_row("k_encrypt_m", "encrypt", [(2, 2048, 0, 4, 33), (1024, 8192, 0, 4, 31)], "k_encrypt_m")
# the ternary add path: K <= 7, one item per wave (ceil(N / 2K) > 32), K values below q on a masked 16-bit field (ME = 2K or K);
# at path 0 only where the matrix path does not apply (q > 8192)
_row("k_encrypt_t<1, 2>", "encrypt", [(65, 16384, 0, 0, 5), (128, 2048, 0, 2, 5)], "k_encrypt_t<1,2>")
_row("k_encrypt_t<1, 1>", "encrypt", [(65, 32768, 0, 0, 5), (128, 32768, 0, 2, 5)], "k_encrypt_t<1,1>")
_row("k_encrypt_t<3, 6>", "encrypt", [(193, 2048, 0, 2, 5), (384, 8192, 0, 2, 5)], "k_encrypt_t<3,6>")
_row("k_encrypt_t<3, 3>", "encrypt", [(193, 16384, 0, 0, 5), (384, 16384, 0, 0, 5)], "k_encrypt_t<3,3>")
_row("k_encrypt_t<5, 10>", "encrypt", [(385, 2048, 0, 2, 5), (640, 4096, 0, 2, 5)], "k_encrypt_t<5,10>")
_row("k_encrypt_t<5, 5>", "encrypt", [(385, 8192, 0, 2, 5), (640, 8192, 0, 3, 5)], "k_encrypt_t<5,5>")
_row("k_encrypt_t<7, 14>", "encrypt", [(641, 2048, 0, 2, 5), (896, 4096, 0, 2, 5)], "k_encrypt_t<7,14>")
_row("k_encrypt_t<7, 7>", "encrypt", [(641, 8192, 0, 2, 5), (896, 8192, 0, 2, 5)], "k_encrypt_t<7,7>")
# the multiply-accumulate kernels: everything else (q = 65536 leaves no field budget for the add path)
_row("k_encrypt<1>", "encrypt", [(2, 2048, 0, 0, 1), (128, 65536, 0, 0, 3)], "k_encrypt<1>")
_row("k_encrypt<3>", "encrypt", [(129, 65536, 0, 0, 3), (384, 2048, 0, 1, 3)], "k_encrypt<3>")
_row("k_encrypt<5>", "encrypt", [(385, 65536, 0, 0, 3), (640, 2048, 0, 1, 3)], "k_encrypt<5>")
_row("k_encrypt<7>", "encrypt", [(641, 65536, 0, 0, 3), (896, 2048, 0, 1, 3)], "k_encrypt<7>")
_row("k_encrypt<9>", "encrypt", [(1025, 2048, 0, 0, 3), (1152, 65536, 0, 0, 3)], "k_encrypt<9>")
_row("k_encrypt<11>", "encrypt", [(1153, 2048, 0, 0, 3), (1408, 8192, 0, 0, 3)], "k_encrypt<11>")
_row("k_encrypt<13>", "encrypt", [(1409, 4096, 0, 0, 3), (1664, 65536, 0, 0, 3)], "k_encrypt<13>")
_row("k_encrypt<15>", "encrypt", [(1665, 2048, 0, 0, 3), (1920, 2048, 0, 0, 3)], "k_encrypt<15>")

# ---- decrypt (p = 3 unless stated) ----------------------------------------------------------------------------------------------
_row("k_decrypt_m8", "decrypt", [(513, 2048, 3, 0, 95), (864, 4096, 3, 0, 97)], "k_decrypt_m8")
_row("k_decrypt_m", "decrypt", [(2, 2048, 3, 4, 33), (1024, 8192, 3, 0, 95), (128, 4096, 3, 4, 33)], "k_decrypt_m")
# shared stepping: paths 2 and 3, odd N, K = ceil(N / 64) made odd in 9..13; ME = K for q <= 4096, 7 at q = 8192 (not for K = 13);
# the dot8 second product where the item takes 32 lanes (ceil(N / 2K) == 32), K >= 11 and path != 3
_row("k_decrypt_s<9, 9, false>", "decrypt", [(449, 2048, 3, 2, 3), (575, 4096, 3, 2, 3)], "k_decrypt_s<9,9>")
_row("k_decrypt_s<9, 7, false>", "decrypt", [(449, 8192, 3, 2, 3), (575, 8192, 3, 2, 3)], "k_decrypt_s<9,7>")
_row("k_decrypt_s<11, 11, false>", "decrypt", [(577, 2048, 3, 2, 3), (703, 4096, 3, 3, 3)], "k_decrypt_s<11,11>")
_row("k_decrypt_s<11, 11, true>", "decrypt", [(683, 2048, 3, 2, 3), (703, 4096, 3, 2, 3)], "k_decrypt_s+dot8<11,11>")
_row("k_decrypt_s<11, 7, false>", "decrypt", [(577, 8192, 3, 2, 3), (703, 8192, 3, 3, 3)], "k_decrypt_s<11,7>")
_row("k_decrypt_s<11, 7, true>", "decrypt", [(683, 8192, 3, 2, 3), (703, 8192, 3, 2, 3)], "k_decrypt_s+dot8<11,7>")
_row("k_decrypt_s<13, 13, false>", "decrypt", [(705, 2048, 3, 2, 3), (831, 4096, 3, 3, 3)], "k_decrypt_s<13,13>")
_row("k_decrypt_s<13, 13, true>", "decrypt", [(807, 2048, 3, 2, 3), (831, 4096, 3, 2, 3)], "k_decrypt_s+dot8<13,13>")
# per-item stepping: path 2 only, the add path's rule (even N where the shared stepping would take odd N)
_row("k_decrypt_t<1, 2>", "decrypt", [(65, 2048, 3, 2, 5), (128, 16384, 3, 2, 5)], "k_decrypt_t<1,2>")
_row("k_decrypt_t<1, 1>", "decrypt", [(65, 32768, 3, 2, 5), (128, 32768, 3, 2, 5)], "k_decrypt_t<1,1>")
_row("k_decrypt_t<3, 6>", "decrypt", [(193, 2048, 3, 2, 5), (384, 8192, 3, 2, 5), (193, 4096, 3, 2, 5)], "k_decrypt_t<3,6>")
_row("k_decrypt_t<3, 3>", "decrypt", [(193, 16384, 3, 2, 5), (384, 16384, 3, 2, 5)], "k_decrypt_t<3,3>")
_row("k_decrypt_t<5, 10>", "decrypt", [(385, 2048, 3, 2, 5), (640, 4096, 3, 2, 5)], "k_decrypt_t<5,10>")
_row("k_decrypt_t<5, 5>", "decrypt", [(385, 8192, 3, 2, 5), (640, 8192, 3, 2, 5)], "k_decrypt_t<5,5>")
_row("k_decrypt_t<7, 14>", "decrypt", [(642, 2048, 3, 2, 5), (896, 4096, 3, 2, 5)], "k_decrypt_t<7,14>")
_row("k_decrypt_t<7, 7>", "decrypt", [(642, 8192, 3, 2, 5), (896, 8192, 3, 2, 5)], "k_decrypt_t<7,7>")
_row("k_decrypt<1>", "decrypt", [(2, 2048, 3, 0, 1), (128, 65536, 5, 0, 3)], "k_decrypt<1>")
_row("k_decrypt<3>", "decrypt", [(129, 65536, 3, 0, 3), (384, 2048, 7, 0, 3)], "k_decrypt<3>")
_row("k_decrypt<5>", "decrypt", [(385, 65536, 3, 0, 3), (640, 8192, 11, 0, 3)], "k_decrypt<5>")
_row("k_decrypt<7>", "decrypt", [(641, 65536, 3, 0, 3), (896, 2048, 3, 1, 3)], "k_decrypt<7>")
_row("k_decrypt<9>", "decrypt", [(1025, 2048, 3, 0, 3), (1152, 8192, 5, 0, 3)], "k_decrypt<9>")
_row("k_decrypt<11>", "decrypt", [(1153, 2048, 3, 0, 3), (1408, 65536, 7, 0, 3)], "k_decrypt<11>")
_row("k_decrypt<13>", "decrypt", [(1409, 4096, 3, 0, 3), (1664, 2048, 5, 0, 3)], "k_decrypt<13>")
_row("k_decrypt<15>", "decrypt", [(1665, 2048, 3, 0, 3), (1920, 8192, 5, 0, 3)], "k_decrypt<15>")

# ---- fused and packed forms -----------------------------------------------------------------------------------------------------
_row("k_decrypt_mp", "decrypt_pack", [(97, 2048, 3, 0, 33), (821, 4096, 3, 0, 95)], "k_decrypt_mp")
_row("k_encrypt_wp<11>", "encrypt_pack", [(64, 2048, 0, 0, 33), (509, 2048, 0, 0, 95)], None,
     "q == 2048, d_e NULL, the row-image kernel's range")
_row("k_encrypt_wp<12>", "encrypt_pack", [(64, 4096, 0, 0, 33), (821, 4096, 0, 0, 95)], None,
     "q == 4096, d_e NULL, the row-image kernel's range")
_row("k_encrypt_wp<13>", "encrypt_pack", [(64, 8192, 0, 0, 33), (701, 8192, 0, 0, 95)], None,
     "q == 8192, d_e NULL, the row-image kernel's range")
_row("k_pack_bytes2", "pack_bytes", [(1, 2, 0, 0, 1), (821, 3, 0, 0, 7)], None, "bits == 2 (max_val 2 or 3)")
_row("k_pack<unsigned char>", "pack_bytes", [(1, 4, 0, 0, 1), (821, 255, 0, 0, 7)], None, "bits != 2")
_row("k_pack<unsigned short>", "pack", [(1, 1, 0, 0, 1), (821, 4095, 0, 0, 7)], None, "every ntru_pack_batch_dev call")
_row("k_unpack", "unpack", [(3, 1, 0, 0, 1), (7, 4095, 0, 0, 7)], None,
     "every ntru_unpack_batch_dev call (N = packed_size, packed_bits 252)")

# ---- verify_keys ----------------------------------------------------------------------------------------------------------------
_row("k_verify_keys_m", "verify_keys", [(128, 2048, 3, 0, 3), (1024, 8192, 3, 0, 3)], "k_verify_keys_m")
_row("k_verify_keys_t<1, 2>", "verify_keys", [(65, 2048, 3, 0, 5), (128, 16384, 3, 0, 5)], "k_verify_keys_t<1,2>")
_row("k_verify_keys_t<1, 1>", "verify_keys", [], "k_verify_keys_t<1,1>",
     unreachable="ME = 1 at K = 1 needs q = 32768, and verify_keys refuses p (q - 1) > 65535; it is instantiated by the "
                 "shared add-path dispatch")
_row("k_verify_keys_t<3, 6>", "verify_keys", [(193, 2048, 3, 2, 5), (384, 8192, 3, 2, 5)], "k_verify_keys_t<3,6>")
_row("k_verify_keys_t<3, 3>", "verify_keys", [(193, 16384, 3, 0, 5), (384, 16384, 3, 0, 5)], "k_verify_keys_t<3,3>")
_row("k_verify_keys_t<5, 10>", "verify_keys", [(385, 2048, 3, 2, 5), (640, 4096, 3, 2, 5)], "k_verify_keys_t<5,10>")
_row("k_verify_keys_t<5, 5>", "verify_keys", [(385, 8192, 3, 2, 5), (640, 8192, 3, 3, 5)], "k_verify_keys_t<5,5>")
_row("k_verify_keys_t<7, 14>", "verify_keys", [(641, 2048, 3, 2, 5), (896, 4096, 3, 2, 5)], "k_verify_keys_t<7,14>")
_row("k_verify_keys_t<7, 7>", "verify_keys", [(641, 8192, 3, 2, 5), (896, 8192, 3, 2, 5)], "k_verify_keys_t<7,7>")
_row("k_verify_keys<1>", "verify_keys", [(2, 2048, 3, 0, 1), (128, 2048, 3, 1, 3)], "k_verify_keys<1>")
_row("k_verify_keys<3>", "verify_keys", [(129, 2048, 3, 1, 3), (384, 8192, 5, 0, 3)], "k_verify_keys<3>")
_row("k_verify_keys<5>", "verify_keys", [(385, 2048, 3, 1, 3), (640, 4096, 11, 0, 3)], "k_verify_keys<5>")
_row("k_verify_keys<7>", "verify_keys", [(641, 2048, 3, 1, 3), (896, 8192, 7, 0, 3)], "k_verify_keys<7>")
_row("k_verify_keys<9>", "verify_keys", [(1025, 2048, 3, 0, 3), (1152, 8192, 5, 0, 3)], "k_verify_keys<9>")
_row("k_verify_keys<11>", "verify_keys", [(1153, 2048, 3, 0, 3), (1408, 8192, 7, 0, 3)], "k_verify_keys<11>")
_row("k_verify_keys<13>", "verify_keys", [(1409, 4096, 3, 0, 3), (1664, 2048, 5, 0, 3)], "k_verify_keys<13>")
_row("k_verify_keys<15>", "verify_keys", [(1665, 2048, 3, 0, 3), (1920, 8192, 5, 0, 3)], "k_verify_keys<15>")

# ---- polymul_split and the public key ---------------------------------------------------------------------------------------
_row("k_polymul_m<true>", "polymul_split", [(64, 256, 0, 4, 3), (1024, 2, 0, 0, 3)], "k_polymul_m")
_row("k_polymul_m<false>", "polymul_split", [(128, 512, 0, 0, 3), (1024, 8192, 0, 0, 3)], "k_polymul_m")
for _K, (_lo, _hi) in K_RANGES.items():
    _row("k_polymul_split<%d, false>" % _K, "polymul_split", [(_lo, 65536, 0, 0, 3), (_hi, 3, 0, 1, 3)],
         "k_polymul_split<%d>" % _K)
_row("k_product_tern_m<true>", "public_key", [(64, 256, 3, 4, 3), (1024, 2, 1, 0, 3)], "k_public_key_m")
_row("k_product_tern_m<false>", "public_key", [(128, 512, 3, 0, 3), (1024, 8192, 8, 0, 3)], "k_public_key_m")
for _K, (_lo, _hi) in K_RANGES.items():
    _row("k_polymul_split<%d, true>" % _K, "public_key", [(_lo, 16384, 3, 0, 3), (_hi, 8192, 5, 1, 3)], "k_public_key<%d>" % _K)

# ---- key inversion (q = 2048, p = 3) --------------------------------------------------------------------------------------------
# register-resident planes for nw = (N + 32) / 32 words up to NWC, planes in LDS (NWC = 0) above the largest case
_INV = {2: (2, 63), 6: (64, 191), 12: (192, 383), 16: (384, 511), 22: (512, 703), 26: (704, 831)}
for _P in (2, 3):
    for _W, (_lo, _hi) in _INV.items():
        _row("k_invert_key<%d, %d>" % (_P, _W), "invert_key", [(_lo, 2048, 3, 0, 3), (_hi, 2048, 3, 0, 3)], None,
             "nw = (N + 32) / 32 <= %d, above the next smaller case" % _W)
_row("k_invert_key<2, 32>", "invert_key", [(832, 2048, 3, 0, 3), (1023, 2048, 3, 0, 3)], None, "27 <= nw = (N + 32) / 32 <= 32")
_row("k_invert_key<2, 0>", "invert_key", [(1024, 2048, 3, 0, 3), (1100, 2048, 3, 0, 3)], None, "nw = (N + 32) / 32 > 32")
_row("k_invert_key<3, 0>", "invert_key", [(832, 2048, 3, 0, 3), (1023, 2048, 3, 0, 3)], None, "nw = (N + 32) / 32 > 26")
_row("k_newton_round_m", "invert_key", [(128, 2048, 3, 0, 3), (1024, 8192, 3, 0, 3)], None,
     "every Newton round on the per-item matrix kernels: 128 <= N <= 1024, q <= 8192")
_row("k_signed_to_u16", "invert_key", [(17, 32, 3, 0, 3), (101, 2048, 3, 0, 3)], None,
     "a Newton round outside the matrix range (N < 128 at path 0)")
_row("k_newton_combine_vec", "invert_key", [(17, 32, 3, 0, 3), (101, 2048, 3, 0, 3)], None,
     "a Newton round outside the matrix range on 16-byte aligned rows, B N >= 8")
_row("k_newton_combine", "invert_key", [(17, 32, 3, 0, 3), (101, 2048, 3, 0, 1)], None,
     "a Newton round outside the matrix range, B N not a multiple of 8")
_row("k_or_bytes", "invert_key", [(17, 32, 3, 0, 3), (821, 4096, 3, 0, 3)], None, "fq and fp both asked for")

# ---- sampler, elementwise, generic ----------------------------------------------------------------------------------------------
for _DR, _R in ((10, 20), (6, 12), (4, 8)):
    _row("k_sample_ternary<false, 4, %d, ConsecutiveItems>" % _DR, "sample_ternary", [(2, 0, _R, 0, 1), (1920, 0, _R, 0, 257)], None,
         "N + 1 < 2048, %d rounds" % _R)
    _row("k_sample_ternary<true, 1, %d, ConsecutiveItems>" % _DR, "sample_ternary", [(2047, 0, _R, 0, 3), (2500, 0, _R, 0, 3)], None,
         "N + 1 >= 2048, %d rounds" % _R)
_row("k_add_mod_vec<true>", "add", [(8, 2048, 0, 0, 1), (821, 65536, 0, 0, 9)], None, "power-of-two mod, 16-byte aligned, B N >= 8")
_row("k_add_mod_vec<false>", "add", [(8, 3, 0, 0, 1), (821, 5, 0, 0, 9)], None, "other mod, 16-byte aligned, B N >= 8")
_row("k_add_mod", "add", [(1, 2, 0, 0, 1), (821, 2048, 0, 0, 9)], None, "B N not a multiple of 8 (or unaligned)")
_row("k_split_by_I", "split_by_I", [(1, 2, 0, 0, 1), (821, 4096, 0, 0, 9)], None, "every ntru_split_by_I_dev call")
_row("(anonymous namespace)::k_generic", "generic_multiply", [(1, 1 << 20, 0, 0, 1), (300, 1 << 20, 0, 0, 5)], "k_generic")

# ---- one key pair per item (matrix_peritem_scheme.hip) ----------------------------------------------------------------------------
_row("k_encrypt_pi_m<true>", "encrypt_peritem", [(64, 256, 0, 4, 7), (128, 32, 0, 0, 7)], "k_encrypt_pi_m", "q <= 256")
_row("k_encrypt_pi_m<false>", "encrypt_peritem", [(128, 512, 0, 0, 7), (1024, 8192, 0, 0, 7)], "k_encrypt_pi_m", "512 <= q <= 8192")
_row("k_decrypt_pi_m<true>", "decrypt_peritem", [(64, 256, 3, 4, 7), (128, 32, 3, 0, 7)], "k_decrypt_pi_m", "q <= 256, p == 3")
_row("k_decrypt_pi_m<false>", "decrypt_peritem", [(128, 512, 3, 0, 7), (1024, 8192, 3, 0, 7), (128, 4096, 3, 0, 7)], "k_decrypt_pi_m",
     "512 <= q <= 8192, p == 3")
# the composed path: N below the matrix range, q above it, a kernel path without the matrix kernels, p != 3 (decrypt)
_COMPOSED = [(2, 2048, 3, 0, 7), (127, 2048, 3, 0, 7), (128, 16384, 3, 0, 7), (128, 2048, 3, 1, 7)]
for _k in ("k_pi_widen", "k_pi_add_bytes"):
    _row(_k, "encrypt_peritem", [(N, q, 0, path, B) for (N, q, _p, path, B) in _COMPOSED], "peritem_composed(k_polymul_split<1>)",
         "composed encrypt")
for _k in ("k_pi_signed_modq", "k_pi_lift", "k_pi_narrow"):
    _row(_k, "decrypt_peritem", _COMPOSED + [(128, 2048, 5, 0, 7)], "peritem_composed(k_polymul_split<1>)", "composed decrypt")

# ---- segmented sums (ciphertext_sum.hip) ----------------------------------------------------------------------------------------
_NS = "(anonymous namespace)::"
for _P2, _mod in ((True, 2048), (False, 65521)):
    for _WT in (False, True):
        _row(_NS + "k_sum_groups<%s, %s>" % (str(_P2).lower(), str(_WT).lower()), "sum_groups",
             [(2, _mod, 0, 0, 6, dict(K=3, weights=_WT)), (513, _mod, 0, 0, 80, dict(K=40, weights=_WT))],
             "k_sum_groups<%d,%d>" % (_P2, _WT), "power-of-two mod: %s, weights: %s; N = 513 is two column tiles" % (_P2, _WT))
    # uniform: the block count is clamped to the row count, so one group of 3 rows crosses two boundaries and one of 40 walks the
    # 32-slice loop twice; offsets form: 4100 rows at N = 17 give blocks of more than one row
    _row(_NS + "k_sum_groups_finish<%s>" % str(_P2).lower(), "sum_groups",
         [(2, _mod, 0, 0, 3, dict(K=3)), (513, _mod, 0, 0, 40, dict(K=40)), (17, _mod, 0, 0, 4100, dict(csr=True))], None,
         "a group crossing a row-block boundary, power-of-two mod: %s" % _P2)

# ---- byte messages (message_bytes.hip) ------------------------------------------------------------------------------------------------
_BYTES = [(8, 0, 0, 0, 5, dict(nbytes=1)), (821, 0, 0, 0, 5, dict(nbytes=102)), (1920, 0, 0, 0, 5, dict(nbytes=1))]
_row(_NS + "k_bytes_to_rows", "bytes_to_rows", _BYTES, "k_bytes_to_rows", "every ntru_bytes_to_rows_dev call")
_row(_NS + "k_rows_to_bytes", "rows_to_bytes", _BYTES, "k_rows_to_bytes", "every ntru_rows_to_bytes_dev call")

# ---- witness checks (witness_check.hip) -------------------------------------------------------------------------------------------------
for _t in ("encrypt", "decrypt", "inverse"):
    _row(_NS + "k_check_" + _t, "check_" + _t, [(2, 32, 3, 0, 3), (821, 4096, 3, 0, 3)], "k_check_" + _t,
         "every ntru_check_%s_batch_dev call" % _t)

# ---- key generation (keygen_batch.hip): the redraw kernels run only when a first draw is a non-unit -----------------------------------
_KEYGEN = [(7, 32, 3, 0, 16, dict(df=2, dg=2, first=125)), (17, 32, 3, 0, 8, dict(df=3, dg=2, first=311))]
for _k in ("k_keygen_compact", "k_keygen_scatter", "k_keygen_finalize"):
    _row(_NS + _k, "keygen", _KEYGEN, "k_keygen", "ntru_keygen_batch_dev with a non-unit among the first draws")
# the sampler at listed positions (ternary_sampler.hip); at the third shape about half of the 256 first draws are non-units: full
# blocks of 64 compact rows with N >= 16, which leave through the aligned output stage (first = 2: the runner's third call starts at 0)
_row("k_sample_ternary<false, 4, 10, ListedItems>", "keygen", _KEYGEN + [(16, 32, 3, 0, 256, dict(df=3, dg=2, first=2))], "k_keygen",
     "ntru_keygen_batch_dev with a non-unit among the first draws")

# ---- packed ciphertexts (packed_ciphertexts.hip) ------------------------------------------------------------------------------------------
SP_BATCH, SP_WAVES_PER_CU = 4, 8      # row steps in flight and waves per CU of k_sum_groups_packed, as the kernel file sets them


def packed_layout(bits, N):
    """How k_sum_groups_packed lays a row of `bits`-wide fields out, restated from per = 252 // bits: os elements of `slices` units, U
    units a row, `side` rows side by side in a wave, NT wavefronts (tiles of 64 units) a row."""
    per = 252 // bits
    os_ = max(-(-N // per), 3)
    slices = (per + 31) // 32 if per > 36 else 1
    U = os_ * slices
    return {"per": per, "os": os_, "slices": slices, "U": U, "side": 64 // U if U <= 32 else 1, "NT": 1 if U <= 64 else -(-U // 64),
            "layout": "side" if U <= 32 else ("row" if U <= 64 else "tiles")}


def packed_shape_ns(bits):
    """{layout: N}, one N per lane layout the width reaches at N <= 1920.  "side" at the smallest row, N = 2 per + 1: os = 3, the third
    element holds one coefficient (nv = 1; for the sliced widths whole units lie behind N), and an unsliced width has side = 21, the
    deepest cross-lane tree and no power of two.  "row" and "tiles" at the smallest N that gives them."""
    per = 252 // bits
    slices = packed_layout(bits, 2)["slices"]
    out = {"side": 2 * per + 1}
    for name, above in (("row", 32), ("tiles", 64)):
        N = (above // slices) * per + 1                     # os = above // slices + 1 elements: the first U above the bound
        if N <= 1920:
            out[name] = N
    return out


def _coprime_from(x, R):
    while math.gcd(x, R) != 1:
        x += 1
    return x


def many_rows_per_block(bits, N, cus):
    """(first row, T, R, Pb, offsets) of one launch of k_sum_groups_packed on a device of `cus` CUs in which every row block holds R
    rows, R = SP_BATCH side + side + 1: the four-step loop, the one-step loop and a last step of fewer than `side` rows all run inside a
    block (launches of at most Pb rows have one row per block, and k_sum_groups_finish does all the adding).  Pb as launch_sum_packed
    computes it (sum_row_blocks), R as cut_of does.  The offsets start behind row 0 and hold a group across several block boundaries,
    empty groups, and groups of sizes coprime to R, which lie wholly inside a block (stored from the registers through the lane tree)
    and across one boundary at every phase."""
    lay = packed_layout(bits, N)
    Pb = max(1, min(32768, cus * SP_WAVES_PER_CU // lay["NT"]))
    side = lay["side"]
    R = SP_BATCH * side + side + 1
    T = (R - 1) * Pb + 1
    first = 3
    sizes = [3 * R + 1, 0, 0]
    cycle = [R - 1, _coprime_from(R // 2, R), 1, 0, R + 1, _coprime_from(2 * side + 1, R)]
    total, i = sum(sizes), 0
    while total < T:
        sizes.append(min(cycle[i % len(cycle)], T - total))
        total += sizes[-1]
        i += 1
    off = first + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    assert off[-1] - off[0] == T and T > Pb and -(-T // Pb) == R, (T, Pb, R)
    size = np.diff(off)
    lo, hi = (off[:-1] - first) // R, (off[1:] - 1 - first) // R            # first and last block of a group that is not empty
    inside, across = (size > 0) & (lo == hi), (size > 0) & (hi == lo + 1)
    assert (size == 0).any() and inside.any() and across.any() and (hi > lo + 2).any(), (bits, N, cus)
    assert (size[inside] >= SP_BATCH * side + side).any(), (bits, N, cus)     # a group inside a block runs the four-step loop and the other
    assert side == 1 or (size[inside] % side != 0).any(), (bits, N, cus)      # and one ends on a step of fewer than `side` rows
    return first, T, R, Pb, off


for _bits in range(1, 17):
    for _P2 in (True, False):
        if _bits == 1 and not _P2:
            continue                                        # mod = 2 is a power of two
        # no power of two: the largest modulus of the width, and the smallest, which a raw field exceeds by almost a factor of two
        _mods = [1 << _bits] if _P2 else sorted({(1 << _bits) - 1, (1 << (_bits - 1)) + 1}, reverse=True)
        for _WT in (False, True):
            _row(_NS + "k_sum_groups_packed<%d, %s, %s>" % (_bits, str(_P2).lower(), str(_WT).lower()), "sum_groups_packed",
                 [(_N, _mod, 0, 0, 0, dict(layout=_lay, weights=_WT)) for _lay, _N in packed_shape_ns(_bits).items() for _mod in _mods],
                 "k_sum_groups_packed<%d,%d,%d>" % (_bits, _P2, _WT))
# a field across a 64-bit limb needs a width that does not divide 64; the third element is partial at every shape
_row(_NS + "k_unpack_rows", "decrypt_packed",
     [(2 * (252 // _bits) + 64 // _bits + 2, 1 << _bits, 3, 0, 5) for _bits in range(1, 17)], None,
     "every ntru_decrypt_packed_batch_dev call: every field width the decrypt entry admits (q = 2 .. 65536)")

BY_KERNEL = {r["kernel"]: r for r in ROWS}
assert len(BY_KERNEL) == len(ROWS), "duplicate row"
# every string ntru_engine_last_kernel() may return after a call of the scheme entry points: the rows of these entries only (the
# dispatch sweep and the p sweeps assert membership, so the set must not grow with the table)
SCHEME_ENTRIES = ("encrypt", "decrypt", "decrypt_pack", "verify_keys", "polymul_split", "public_key", "generic_multiply")
LAST_KERNELS = {r["last"] for r in ROWS if r["last"] and r["entry"] in SCHEME_ENTRIES} | {"k_invert_key", "k_sample_ternary", "k_encrypt_wp"}
assert len(LAST_KERNELS) == 84, len(LAST_KERNELS)

# ---- the lift (both modes on every row of the decrypt family) ---------------------------------------------------------------------------------
LIFT_ENTRIES = ("decrypt", "decrypt_pack", "decrypt_peritem")


def lift_addend(q, p):
    """What the centred lift adds to x > q/2 in place of the reference's 1."""
    return (p - q % p) % p


# These kernels need p = 3, where the addend is 1 for q = 2^odd and 2 for q = 2^even, and their mask interval ME admits one q only:
# 65535 / (q - 1) - 1 must reach ME and stay below the next interval of the same K.
for _k, _why in (("k_decrypt_s<9, 7, false>", "ME = 7 below K = 9: q = 8192 only"),
                 ("k_decrypt_s<11, 7, false>", "ME = 7 below K = 11: q = 8192 only"),
                 ("k_decrypt_s<11, 7, true>", "ME = 7 below K = 11: q = 8192 only"),
                 ("k_decrypt_t<1, 1>", "ME = 1 and not 2: q = 32768 only"),
                 ("k_decrypt_t<5, 5>", "ME = 5 and not 10: q = 8192 only"),
                 ("k_decrypt_t<7, 7>", "ME = 7 and not 14: q = 8192 only")):
    BY_KERNEL[_k]["addend_one_only"] = _why
