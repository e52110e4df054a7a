#!/usr/bin/env python3
"""Compare the kernels of two sets of raw gfx950 code objects, by name.

    codeobj_diff.py OLD_DIR NEW_DIR

Each directory holds one code object per translation unit, under the same
file names (hipcc <product flags> --offload-device-only --no-gpu-bundle-output
-c -o DIR/sf3.co csrc/lphy_sf.hip -DLPHY_SF=3, ...).  Per kernel: the
register / spill / LDS / scratch / kernarg figures of its metadata note and a
hash of its instruction words.  A kernel whose figures are equal and whose
words differ only in the 32-bit literal added to a register pair within 8
instructions of the s_getpc_b64 that wrote it (the PC-relative address of a
global or callee: it changes when either moved) is reported as "relocated".
Exit status 1 for a different kernel, a kernel only in NEW_DIR, or one that
left its object and is in no object of NEW_DIR.  Hashing and comparing only."""
import hashlib
import re
import subprocess
import sys
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
          ".private_segment_fixed_size", ".group_segment_fixed_size", ".kernarg_segment_size")


def kernels(co):
    notes = subprocess.run([LLVM / "llvm-readobj", "--notes", co], capture_output=True, text=True, check=True).stdout
    meta = {}
    for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
        name = re.search(r"\.symbol:\s+'?([\w.$]+?)\.kd'?\s", blk).group(1)
        meta[name] = tuple(int(re.search(re.escape(f) + r":\s+(\d+)", blk).group(1)) for f in FIELDS)
    dis = subprocess.run([LLVM / "llvm-objdump", "-d", co], capture_output=True, text=True, check=True).stdout
    out, cur, pc = {}, None, {}  # pc: register -> instructions left in its s_getpc_b64 window
    for line in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <([\w.$]+)>:", line)
        if m:
            cur = m.group(1) if m.group(1) in meta else None
            pc = {}
            if cur:
                out[cur] = (meta[cur], hashlib.sha1(), hashlib.sha1())
            continue
        m = re.match(r"\s+(\S+)\s.*// [0-9A-F]+: ((?:[0-9A-F]{8} ?)+)", line) if cur else None
        if m:
            words = m.group(2).split()
            out[cur][1].update(" ".join(words).encode())
            # the same with the 32-bit literal of a PC-relative add masked
            pc = {r: n - 1 for r, n in pc.items() if n > 1}
            g = re.search(r"s_getpc_b64 s\[(\d+):(\d+)\]", line)
            if g:
                pc[g.group(1)] = pc[g.group(2)] = 8
            a = re.search(r"s_addc?_u32 s(\d+), s\1, (0x[0-9a-f]+|-?\d+)\s", line)
            pcrel = len(words) == 2 and a and a.group(1) in pc
            out[cur][2].update((words[0] + (" *" if pcrel else " " + " ".join(words[1:]))).encode())
    return {k: (v[0], v[1].hexdigest(), v[2].hexdigest()) for k, v in out.items()}


def main(old_dir, new_dir):
    bad = 0
    new = {p.name: kernels(p) for p in sorted(Path(new_dir).glob("*.co"))}
    anywhere = set().union(*new.values())
    for old in sorted(Path(old_dir).glob("*.co")):
        a, b = kernels(old), new[old.name]
        same = [k for k in a if k in b and a[k][:2] == b[k][:2]]
        reloc = [k for k in a if k in b and a[k][0] == b[k][0] and a[k][1] != b[k][1] and a[k][2] == b[k][2]]
        diff = [k for k in a if k in b and k not in same and k not in reloc]
        gone, added = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        print(f"{old.name}: {len(a)} -> {len(b)} kernels; identical {len(same)}, relocated {len(reloc)}, "
              f"different {len(diff)}, only old {len(gone)}, only new {len(added)}")
        for tag, ks in (("relocated", reloc), ("DIFFERENT", diff), ("only old", gone), ("only new", added)):
            for k in ks:
                print(f"    {tag}: {k}")
        bad += len(diff) + len(added) + len([k for k in gone if k not in anywhere])
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
