"""MI355X-native NTRU polynomial-ring engine: host-side mirror of the reference's hot-path interface.

Layout
  csrc/abi.hip           engine life cycle + the *_dev entry points of the C ABI declared in include/ntru_engine.h
  csrc/valu_families.hip, matrix_encrypt.hip, matrix_decrypt.hip, matrix_peritem.hip, key_inversion.hip, ternary_sampler.hip, elementwise.hip
                         the HIP kernels (gfx950), one translation unit per kernel family (csrc/engine_internal.h lists them)
  csrc/ntru_host.hip     host-pointer entry points: pinned staging, three stage streams, chunked H2D / kernel / D2H pipeline
  csrc/ntru_generic.hip  reference-faithful generic family (arbitrary divisors, moduli up to 2^26, EEA, polyInv)
  lib/libntru_engine.so  built artefact (make -C csrc, or __graft_entry__.build())
  engine.py              ctypes binding of the C ABI (numpy host buffers or raw device pointers)
  lift.py                the lift of decryptBits as a mode of an engine: set_lift, get_lift, using (functions on an Engine / MultiEngine)
  packed.py              sums, tallies and decrypts of ciphertexts that arrive as packOutput rows (functions on an Engine)
  csrc/permutation.hip   the order of a mix step drawn on the device (ChaCha20 sort keys + a stable radix argsort), one call per mix step
  mix.py                 re-randomising and shuffling ciphertexts under the shared public key, the order drawn on the device, a whole
                         mix step from a key (functions on an Engine)
  csrc/matrix_combine.hip  G linear combinations of the same rows by a weight matrix, on the matrix cores (k_combine_m) or the vector ALU
  combine.py             combining ciphertexts by a weight matrix: out = weights^T . rows (functions on an Engine)
  csrc/matrix_mulshared.hip  a batch of full-range rows times one shared full-range polynomial, on the matrix cores (k_mul_shared_m)
  shared_product.py      multiplying a batch by one shared polynomial, with the split by 1 - x^N (functions on an Engine)
  csrc/matrix_noise.hip  the decryption noise of rows under a key: decrypt's first product reduced to peak and energy (k_noise_m)
  noise.py               measuring noise: peak = max |a centred|, energy = sum of squares, per row, dense or packed (functions on an Engine)
  csrc/dedup_rows.hip    the duplicate rows of a batch: keyed fingerprints, the stable argsort, one exact neighbour comparison, compaction
  dedup.py               removing duplicates: first occurrence and unique list of a batch against a prior set, dense or packed (functions on an
                         Engine)
  csrc/mix_audit.hip     checking revealed re-encryption links: the encrypt body with a compare in the place of the stores (k_linkcheck_m)
  audit.py               auditing a mix: check_links, and randomized partial checking of a pair of mix steps (functions on an Engine)
  scan.py                scanning a batch for the rows a key decrypts to a tagged message; only the hits come back (functions on an Engine)
  csrc/count_bytes.hip   the decrypted byte messages of a batch classified on the device and counted by choice and group (k_count_classify)
  count.py               counting decrypted messages: count [G][n_choices + 3] and optional per-row classes, dense or packed (functions on
                         an Engine)
  ntru.py                `NTRU` class + pure functions with the reference's names and semantics (index.js)
  js/                    N-API addon + ES-module shim exposing the same surface to Node.js

There is no CPU implementation in this package: everything that computes goes through the HIP library and
raises `EngineError` when it (or a GPU) is missing.
"""
from .engine import (FLAG_NOT_BITS, FLAG_PAD_NONZERO, Engine, EngineError, MultiEngine, library_path,  # noqa: F401
                     load_library)
from . import audit, combine, count, dedup, lift, mix, noise, packed, scan, shared_product, sharding  # noqa: F401
from .combine import combine_batch, combine_batch_dev  # noqa: F401
from .shared_product import mul_shared_batch, mul_shared_batch_dev  # noqa: F401
from .noise import noise_batch, noise_batch_dev, noise_packed_batch, noise_packed_batch_dev  # noqa: F401
from .dedup import dedup_packed, dedup_packed_dev, dedup_rows, dedup_rows_dev, dedup_workspace_bytes  # noqa: F401
from .mix import reencrypt_batch, reencrypt_batch_dev  # noqa: F401
from .audit import check_links, check_links_dev, open_links, verify_rpc  # noqa: F401
from .mix import (argsort_keys_dev, draw_permutation, draw_permutation_dev, mix_batch, mix_batch_dev)  # noqa: F401
from .scan import (scan_bytes_batch, scan_bytes_batch_dev, scan_bytes_packed_batch,  # noqa: F401
                   scan_bytes_packed_batch_dev)
from .count import (count_bytes_batch, count_bytes_batch_dev, count_bytes_packed_batch,  # noqa: F401
                    count_bytes_packed_batch_dev)
from .packed import (decrypt_packed_batch, decrypt_packed_batch_dev, pack_rows, sum_groups_packed,  # noqa: F401
                     sum_groups_packed_dev, tally_decrypt_packed_batch, tally_decrypt_packed_batch_dev, unpack_rows)
from .ntru import (NTRU, addCiphertexts, addPolynomials, bigintToBits, bitsToBigInt, bitsToString, degree,  # noqa: F401
                   dividePolynomials, expandArray, extendedEuclideanAlgorithm, generateCustomArray, modInverse,
                   multiplyPolynomials, multiplyPolynomialsByScalar, packOutput, polyInv, stringToBits, checkWitnesses,
                   combineCiphertexts, subtractPolynomials, sumCiphertexts, trimPolynomial, unpackInput)
