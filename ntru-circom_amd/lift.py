"""The lift of decryptBits, a mode of the engine (include/ntru_engine.h "The lift of decryptBits"; INTEGRATION.md "The lift").

  "reference" (0)   index.js:117 verbatim, x > q/2 ? (x + 1) % p : x % p: the default, bit-identical to the reference, and what the
                    VerifyDecrypt circuit accepts as a witness.
  "centred"   (1)   x > q/2 ? (x - q) mod p : x % p, the addend (p - q % p) % p in place of 1: returns the plaintext where the
                    reference's + 1 does not (q = 4096 with p = 3; almost every q with p = 5 or 7).  VerifyDecrypt accepts a centred
                    witness only when that addend is 1, where both modes give the same bytes.

Functions on an Engine or a MultiEngine: their classes keep the methods they had.  The mode is read when a call enqueues; do not
change it while a host-form call on that engine is running."""
import contextlib

from .engine import MultiEngine

REFERENCE, CENTRED = 0, 1
MODES = {"reference": REFERENCE, "centred": CENTRED, REFERENCE: REFERENCE, CENTRED: CENTRED}


def addend(mode, q, p):
    """What the lift adds to x > q/2 before the reduction mod p."""
    return (p - q % p) % p if mode_number(mode) == CENTRED else 1


def mode_number(mode):
    """0 / 1 of "reference" / "centred" / 0 / 1; anything else is a ValueError before any library call."""
    if isinstance(mode, bool) or not isinstance(mode, (str, int)) or mode not in MODES:
        raise ValueError('lift: unknown mode %r ("reference", "centred", 0 or 1)' % (mode,))
    return MODES[mode]


def set_lift(eng, mode):
    """ntru_engine_set_lift, or ntru_multi_set_lift for every engine of a MultiEngine."""
    mode = mode_number(mode)
    if isinstance(eng, MultiEngine):
        eng._chk(eng._lib.ntru_multi_set_lift(eng._h, mode))
        eng._lift = mode                       # the C ABI has no getter for a multi-device engine: remembered here
    else:
        eng._chk(eng._lib.ntru_engine_set_lift(eng._h, mode))


def get_lift(eng):
    """The mode as 0 (reference) or 1 (centred)."""
    if isinstance(eng, MultiEngine):
        return getattr(eng, "_lift", REFERENCE)
    return int(eng._lib.ntru_engine_get_lift(eng._h))


@contextlib.contextmanager
def using(eng, mode):
    """The engine in `mode` inside the block, in the mode it had before on every way out."""
    mode = mode_number(mode)
    before = get_lift(eng)
    set_lift(eng, mode)
    try:
        yield eng
    finally:
        set_lift(eng, before)
