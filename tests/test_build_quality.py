"""Build-time quality gates for the HIP kernels (CPU only: hipcc cross-compiles gfx950 without a GPU)."""
import os
import re
import subprocess

import __graft_entry__ as ge


import pytest



def _kernel_tus():
    """Every entry of the Makefile's KERNEL_SRCS, without its suffix: a kernel file added to the library is scanned from then on."""
    with open(os.path.join(ge.PKG_DIR, "csrc", "Makefile")) as fh:
        m = re.search(r"^KERNEL_SRCS\s*:?=\s*(.+)$", fh.read(), re.M)
    assert m, "no KERNEL_SRCS line in the Makefile"
    return tuple(os.path.splitext(f)[0] for f in m.group(1).split())


KERNEL_TUS = _kernel_tus()
assert len(KERNEL_TUS) >= 13 and len(set(KERNEL_TUS)) == len(KERNEL_TUS), KERNEL_TUS
# the shipped library: (EXTRA, fewest wide stores the scan must see).  Counted once on the default build's ISA: 173 dwordx3 / dwordx4
# stores in what are now fifteen translation units (matrix_rowimage 108, key_inversion 46, ternary_sampler 6, elementwise 2,
# ciphertext_sum 8, message_bytes 3; packed_ciphertexts has none).  The sampler's listed instantiation has added one since.
BUILDS = {"default": ("", 173)}


@pytest.fixture(scope="module")
def asm_dirs(tmp_path_factory):
    """ASMDIR of each build: fresh for this run, so that no ISA from another checkout or an earlier source is scanned."""
    return {b: str(tmp_path_factory.mktemp("asm_" + b)) for b in BUILDS}


def _asm_usage(build, asm_dir):
    """`make asm` (one .s + one .usage per kernel translation unit under asm_dir, rebuilt when a source is newer); returns
    the concatenated resource-usage remarks."""
    extra, _ = BUILDS[build]
    src = os.path.join(ge.PKG_DIR, "csrc")
    cmd = ["make", "-C", src, "asm", "ASMDIR=" + asm_dir] + (["EXTRA=" + extra] if extra else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    return "".join(open(os.path.join(asm_dir, t + ".usage")).read() for t in KERNEL_TUS)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_no_kernel_spills_to_scratch(build, asm_dirs):
    """Register spills go to scratch memory = extra HBM traffic (round 1 measured 2.7-3.2x the algorithmic bytes
    before they were removed): every kernel must report ScratchSize 0."""
    text = _asm_usage(build, asm_dirs[build])
    names = re.findall(r"Function Name: (\S+)", text)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", text)]
    assert len(names) == len(scratch) and len(names) >= 40, (len(names), len(scratch))
    bad = [(n, s) for n, s in zip(names, scratch) if s]
    assert not bad, bad
    for must in ("k_encrypt_t", "k_decrypt_s", "k_encrypt", "k_decrypt", "k_verify_keys", "k_polymul_split", "k_encrypt_wp", "k_decrypt_mp",
                 "k_check_decrypt", "k_keygen_scatter", "k_decrypt_pi_m", "k_sum_groups_finish", "k_rows_to_bytes", "k_sum_groups_packed",
                 "k_unpack_rows"):
        assert any(must in n for n in names), must


def _store_data_registers(line):
    """(lo, hi) of the data operand of a 12- or 16-byte store.  buffer_store takes the data first (`buffer_store_dwordx4 v[4:7], v0,
    s[8:11], 0 offen`); global / flat / scratch take the address first, and with a 64-bit vector address that is a register pair of its
    own (`global_store_dwordx4 v[32:33], v[36:39], off`): the data is the second vector operand."""
    m = re.search(r"\b(buffer|global|flat|scratch)_store_dwordx[34]\s+(.*)$", line)
    ops = [o.strip() for o in m.group(2).split(",")]
    data = ops[0] if m.group(1) == "buffer" else ops[1]
    r = re.fullmatch(r"v\[(\d+):(\d+)\]", data)
    assert r, ("no data register range in", line)
    assert int(r.group(2)) - int(r.group(1)) in (2, 3), line
    return int(r.group(1)), int(r.group(2))


def test_store_data_registers_reads_the_data_operand():
    assert _store_data_registers("\tglobal_store_dwordx4 v[32:33], v[36:39], off") == (36, 39)
    assert _store_data_registers("\tglobal_store_dwordx3 v0, v[1:3], s[2:3] offset:4") == (1, 3)
    assert _store_data_registers("\tflat_store_dwordx4 v[10:11], v[2:5]") == (2, 5)
    assert _store_data_registers("\tscratch_store_dwordx4 off, v[4:7], s0") == (4, 7)
    assert _store_data_registers("\tbuffer_store_dwordx4 v[4:7], v0, s[8:11], 0 offen") == (4, 7)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_no_wide_store_followed_by_a_write_of_its_data_registers(build, asm_dirs):
    """gfx950, measured (profiles/archive/r02_hazard_store_x4_soffset.txt): a buffer_store_dwordx4 whose data registers the very next
    instruction overwrites can store the NEW value of the first dword when the memory pipe is busy.  The compiler separates
    the two only when the store's soffset is not a register, so the kernels never pass a scalar offset to their 16-byte
    stores; this scans the generated ISA of every kernel translation unit for the pattern."""
    _asm_usage(build, asm_dirs[build])
    lines = []
    for t in KERNEL_TUS:
        lines += open(os.path.join(asm_dirs[build], t + ".s")).read().split("\n")
    kern, n, bad = None, 0, []
    for i, line in enumerate(lines):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            kern = m.group(1)
        if not re.search(r"\b(buffer|global|flat|scratch)_store_dwordx[34]\b", line):
            continue
        lo, hi = _store_data_registers(line)
        j = i + 1
        while j < len(lines) and (lines[j].strip().startswith(";") or not lines[j].strip() or re.match(r"^\.?\w+:", lines[j].strip())):
            j += 1                                            # comments, blank lines and labels (.LBB0_3:) are not instructions
        nxt = lines[j].strip()
        n += 1
        w = re.match(r"^v_\w+\s+v\[?(\d+)(?::(\d+))?", nxt)
        if w and not nxt.startswith(("v_cmp", "v_cmpx")):
            a = int(w.group(1)); b = int(w.group(2) or a)
            if not (b < lo or a > hi):
                bad.append((kern, line.strip(), nxt))
    assert n >= BUILDS[build][1], n                       # the scan saw the wide stores of this build
    assert not bad, bad[:5]


def _instantiation(demangled):
    """`void k_decrypt_s<11, 11, true>(Geom, ...)` -> `k_decrypt_s<11, 11, true>`: return type and argument list dropped."""
    depth = 0
    for i in range(len(demangled) - 1, -1, -1):
        depth += {")": 1, "(": -1}.get(demangled[i], 0)
        if demangled[i] == "(" and depth == 0:
            demangled = demangled[:i]
            break
    return demangled[5:] if demangled.startswith("void ") else demangled


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_every_kernel_instantiation_has_a_variant_row(build, asm_dirs):
    """tests/kernel_variants.py has one row per compiled kernel instantiation, and names no other: a template case added to a
    dispatch without a test row that launches it fails here, on the CPU."""
    import kernel_variants as kv
    mangled = sorted(set(re.findall(r"Function Name: (\S+)", _asm_usage(build, asm_dirs[build]))))
    out = subprocess.run(["/usr/bin/c++filt"], input="\n".join(mangled), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    compiled = {_instantiation(d) for d in out.stdout.split("\n") if d.strip()}
    assert len(compiled) >= 187, len(compiled)               # 100 of the first seven files, 24 of the five newer ones, 63 packed
    rows = [r["kernel"] for r in kv.ROWS]
    assert len(rows) == len(set(rows)), "duplicate rows"
    assert not compiled - set(rows), ("compiled without a row", sorted(compiled - set(rows)))
    assert not set(rows) - compiled, ("row without a compiled instantiation", sorted(set(rows) - compiled))
    for r in kv.ROWS:
        assert bool(r["shapes"]) != bool(r["unreachable"]), r["kernel"]          # a call that launches it, or why there is none
        assert r["last"] or r["rule"], r["kernel"]
