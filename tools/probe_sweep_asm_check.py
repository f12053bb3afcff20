"""Report on the device assembly of the probe kernels: does a sweep's trial run the floating-point instructions of a single fit?

    python3 tools/probe_sweep_asm_check.py bn_probe.hip.s bn_probe_sweep.hip.s [--strict]

csrc/bn_probe_step.h writes every kernel of the training step once, with a compile-time switch between the single fit (SWEEP = false,
instantiated by bn_probe.hip) and the sweep (SWEEP = true, bn_probe_sweep.hip).  The sweep's contract — a trial without label smoothing
has the bits of a single fit — needs more than the same source text: the files are built with floating-point contraction on, and where
the compiler fuses a multiplication into an addition is its own choice per instantiation.  So this compares, kernel by kernel, how often
every floating-point opcode occurs in the two instantiations.  The only difference allowed is the label smoothing of the sweep's
training forward kernel: one multiplication and one addition more per target element a lane holds (4 rows x NT column tiles), and no
fused form fewer; and the integer division that splits the gradient kernel's z into trial and row group, which the compiler does with
a float32 reciprocal.  The forward kernel's instantiations with the focal loss and the row weights (its third template argument, EXT = 1)
are pairs like the others and take the same allowance: their loss arithmetic is written with contraction off, so there is nothing for
the compiler to fuse in one instantiation and not in the other.  The quantisation-aware fine-tune (EXT = 2 and the probe_qat_* kernels)
is a single fit's only and has no pair.  Opcodes are counted without their encoding suffix (_e32 / _e64 / _dpp / _sdwa).  Anything else is printed as a
warning.  No part of the build (`make probe-asm-check` in csrc/ runs it): another compiler may lower these two idioms differently without
touching the arithmetic, and the GPU tests, which compare the bits, hold the contract (tests/test_gpu_probe_sweep.py).  This is where
to look first, on a machine without a GPU, when they fail.  --strict makes a difference the exit status.  Needs c++filt; without it, it says so and checks nothing.
"""

import collections
import re
import subprocess
import sys


def kernels(path):
    """{(base name, template arguments without the SWEEP switch): (is_sweep, Counter of float opcodes)} of one assembly file."""
    out, cur = {}, None
    names = [m.group(1) for m in (re.match(r"^(_Z\w+):", line) for line in open(path)) if m]
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    demangled = dict(zip(names, plain))
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            d = demangled[m.group(1)]
            k = re.match(r"(?:void )?bn::(probe_\w+_kernel)(?:<([^>]*)>)?\(", d)
            if not k:
                cur = None
                continue
            targs = [a.strip() for a in (k.group(2) or "").split(",") if a.strip()]
            cur = (k.group(1), tuple(a for a in targs if a not in ("true", "false")))
            out[cur] = ("true" in targs, collections.Counter())
            continue
        tok = line.split()
        if cur is None or not tok or tok[0][0] in ".;":
            continue
        if tok[0].startswith("v_") and ("f32" in tok[0] or "mfma" in tok[0]):   # float32 arithmetic, comparisons, conversions
            out[cur][1][re.sub(r"_(e32|e64|dpp|sdwa)$", "", tok[0])] += 1
    return out


def main(single_path, sweep_path, strict=False):
    try:
        single, sweep = kernels(single_path), kernels(sweep_path)
    except (OSError, subprocess.CalledProcessError) as exc:
        print(f"probe_sweep_asm_check: not run ({exc})")
        return 0
    bad = 0
    for key, (is_sweep, ops) in sorted(single.items()):
        if key[0] == "probe_fwd_kernel" and key[1][1] == "2":   # scores only (bn_head_forward): no part of a sweep
            continue
        if key[0].startswith("probe_qat_") or (key[0] == "probe_fwd_kernel" and key[1][2] == "2"):   # QAT (EXT = 2): a single fit's only
            continue
        if is_sweep or key not in sweep:
            print(f"probe_sweep_asm_check: no sweep instantiation of {key}" if key not in sweep else f"{key}: a sweep kernel in {single_path}")
            bad += 1
            continue
        got = collections.Counter(sweep[key][1])
        if key[0] == "probe_fwd_kernel" and key[1][1] == "0":   # the smoothing: 4 NT multiplications and additions
            n = 4 * int(key[1][0])
            got["v_mul_f32"] -= n
            got["v_add_f32"] -= n
        if key[0] == "probe_dw_kernel":   # trial = z / groups: the unsigned division goes through a float32 reciprocal
            for op in ("v_cvt_f32_u32", "v_rcp_iflag_f32", "v_mul_f32", "v_cvt_u32_f32"):
                got[op] -= 1
        diff = {op: (ops[op], got[op]) for op in set(ops) | set(got) if ops[op] != got[op]}
        if diff:
            bad += 1
            print(f"probe_sweep_asm_check: warning: {key[0]}<{', '.join(key[1])}> single fit vs sweep: " + ", ".join(f"{op} {a} vs {b}" for op, (a, b) in sorted(diff.items())))
    missing = [k for k in sweep if k not in single and k[0] != "probe_sweep_snapshot_kernel"]
    if missing:
        print(f"probe_sweep_asm_check: sweep kernels without a single-fit twin: {missing}")
        bad += 1
    print(f"probe_sweep_asm_check: {len(single)} kernels, {bad} differing")
    return 1 if bad and strict else 0


if __name__ == "__main__":
    sys.exit(main(*[a for a in sys.argv[1:] if a != "--strict"][:2], strict="--strict" in sys.argv))
