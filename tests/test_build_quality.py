"""Build-time quality gates for the HIP kernels (CPU only: hipcc cross-compiles gfx950 without a GPU)."""
import os
import re
import subprocess

import __graft_entry__ as ge


import pytest

KERNEL_TUS = ("valu_families", "matrix_encrypt", "matrix_decrypt", "matrix_rowimage", "matrix_peritem", "keygen_sampler_pack",
              "ntru_generic")
# the shipped library: (EXTRA, fewest wide stores the scan must see)
BUILDS = {"default": ("", 4)}


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
    for must in ("k_encrypt_t", "k_decrypt_s", "k_encrypt", "k_decrypt", "k_verify_keys", "k_polymul_split", "k_encrypt_wp", "k_decrypt_mp"):
        assert any(must in n for n in names), must


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
        data = re.search(r"v\[(\d+):(\d+)\]", line)
        lo, hi = int(data.group(1)), int(data.group(2))
        j = i + 1
        while j < len(lines) and (lines[j].strip().startswith(";") or not lines[j].strip()):
            j += 1
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
    assert len(compiled) >= 100, len(compiled)
    rows = [r["kernel"] for r in kv.ROWS]
    assert len(rows) == len(set(rows)), "duplicate rows"
    assert not compiled - set(rows), ("compiled without a row", sorted(compiled - set(rows)))
    assert not set(rows) - compiled, ("row without a compiled instantiation", sorted(set(rows) - compiled))
    for r in kv.ROWS:
        assert bool(r["shapes"]) != bool(r["unreachable"]), r["kernel"]          # a call that launches it, or why there is none
        assert r["last"] or r["rule"], r["kernel"]
