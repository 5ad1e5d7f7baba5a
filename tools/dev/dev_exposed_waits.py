#!/usr/bin/env python3
"""Developer aid (CPU only): the exposed global-memory waits of a HIP file's kernels, read from the device assembly.
  python tools/dev/dev_exposed_waits.py csrc/fused_rows.hip [<kernel name fragment> ...] [--brief]
Cross-compiles the file with build.py's flags (device side only, -S) and walks every kernel's listing in order, keeping the
queue the hardware keeps: global loads, stores and float atomics retire in issue order, and `s_waitcnt vmcnt(N)` waits until at
most N of them are outstanding.  Per kernel it lists every `vmcnt(0)` / `vmcnt(1)` that
  L  retires a global_load issued with no v_mfma between the load and the wait (nothing hides that round trip), or
  S  retires a global_store or global_atomic_add_f32 (the wave sits out a write's acknowledgement),
each with its line in the listing, and prints VGPRs, scratch and LDS from the kernel descriptor.  The walk is the straight-line
order of the listing: a loop body counts once, and a branch around a store still counts the store -- read the entry's line.
It reads those five mnemonics and the descriptor fields and nothing else."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from camouflage_multimodal_amd import build as B  # noqa: E402


def assemble(src):
    name = os.path.basename(src)
    out = os.path.join(tempfile.mkdtemp(prefix="exposed_waits_"), name.replace(".hip", ".s"))
    flags = [f for f in B.FLAGS if f != "-fPIC"] + B.EXTRA_FLAGS.get(name, [])
    subprocess.run([B._hipcc(), *flags, "--cuda-device-only", "-S", src, "-o", out], check=True)
    return out


def demangle(sym):
    import shutil
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")      # (without one the mangled symbol is shown, and matched)
    if not tool:
        return sym
    try:
        return subprocess.run([tool, sym], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return sym


def kernels(lines):
    """(symbol, first line, last line) of every kernel: from its label to its .Lfunc_end."""
    syms = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    for s in syms:
        start = next(i for i, l in enumerate(lines) if l.startswith(s + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        yield s, start, end


def descriptor(lines, sym):
    i = next(i for i, l in enumerate(lines) if re.match(rf"\s*\.amdhsa_kernel\s+{re.escape(sym)}\s*$", l))
    d = {}
    for l in lines[i:]:
        if ".end_amdhsa_kernel" in l:
            break
        m = re.match(r"\s*\.amdhsa_(next_free_vgpr|accum_offset|private_segment_fixed_size|group_segment_fixed_size)\s+(\d+)", l)
        if m:
            d[m.group(1)] = int(m.group(2))
    return d


def walk(lines, start, end):
    queue, entries, mfmas = [], [], 0          # queue: (kind, listing line, MFMAs issued before it)
    for n in range(start, end):
        t = lines[n].split(";")[0].split()
        if not t:
            continue
        op = t[0]
        if op.startswith("v_mfma"):
            mfmas += 1
        elif op.startswith("global_load"):
            queue.append(("L", n + 1, mfmas))
        elif op.startswith("global_store") or op.startswith("global_atomic_add_f32"):
            queue.append(("S", n + 1, mfmas))
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", lines[n])
            if not m:
                continue
            keep = int(m.group(1))
            gone = queue[:len(queue) - keep] if keep else queue
            if keep <= 1 and gone:
                bare = [q for q in gone if q[0] == "L" and q[2] == mfmas]
                wr = [q for q in gone if q[0] == "S"]
                if bare or wr:
                    entries.append((n + 1, keep, len(bare), bare[0][1] if bare else 0, len(wr), wr[0][1] if wr else 0))
            queue = queue[len(queue) - keep:] if keep else []
    return entries


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    brief = "--brief" in sys.argv
    src = args[0] if os.path.exists(args[0]) else os.path.join(ROOT, "camouflage_multimodal_amd", args[0])
    frags = args[1:]
    path = src if src.endswith(".s") else assemble(src)
    lines = open(path).read().split("\n")
    print(f"listing: {path}")
    for sym, start, end in kernels(lines):
        name = demangle(sym).replace("(anonymous namespace)::", "").replace("void ", "")
        if frags and not any(f in name for f in frags):
            continue
        d = descriptor(lines, sym)
        ent = walk(lines, start, end)
        nl = sum(1 for e in ent if e[2]); ns = sum(1 for e in ent if e[4])
        print(f"{name}: lines {start + 1}..{end}  VGPRs {d.get('next_free_vgpr')} (accum offset {d.get('accum_offset')})  scratch {d.get('private_segment_fixed_size')} B  "
              f"static LDS {d.get('group_segment_fixed_size')} B  |  waits with bare loads {nl}, behind stores / atomics {ns}")
        if brief:
            continue
        for line, keep, nb, l0, nw, s0 in ent:
            what = []
            if nb:
                what.append(f"L {nb} load(s), no MFMA since (first at {l0})")
            if nw:
                what.append(f"S {nw} store(s) / atomic(s) (first at {s0})")
            print(f"   {line:7d}  vmcnt({keep})  " + ";  ".join(what))


if __name__ == "__main__":
    main()
