#!/usr/bin/env python3
"""Count what a kernel's ISA exposes: python tools/isa_counts.py FILE.s [name-substring]

FILE.s is the device assembly of a translation unit (hipcc <product flags> -S --cuda-device-only csrc/mlp.hip).  For every kernel whose
demangled name contains the substring (default: nerfmlp_dgrad_kernel) one line of counts:
  insts / mfma / gload / gstore   instructions, MFMAs, global loads (LDS-DMA loads included), global stores
  serial                          global loads whose next instruction is s_waitcnt vmcnt(0): a dependent round trip each
  scratch ld/st                   loads from / stores to private memory
  head / gap / tail               longest stretch of instructions without an MFMA before the first one, between two, after the last one
  spill / priv                    .vgpr_spill_count and .private_segment_fixed_size of the kernel's metadata
"""
import re
import subprocess
import sys


def kernels(path):
    text = open(path).read().splitlines()
    body, meta, name = {}, {}, None
    for ln in text:
        s = ln.strip()
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name = m.group(1)
            body[name] = []
        elif s.startswith(".Lfunc_end"):
            name = None
        elif name and s and not s.startswith((".", ";")) and not re.match(r"^[.\w$]+:", s):
            body[name].append(s.split(";")[0].strip())
    cur = None
    for ln in text:
        m = re.match(r"\s*-?\s*\.name:\s+(\S+)", ln)
        if m:
            cur = m.group(1)
        m = re.match(r"\s*-?\s*\.(vgpr_spill_count|private_segment_fixed_size|vgpr_count|agpr_count):\s+(\d+)", ln)
        if m and cur:
            meta.setdefault(cur, {})[m.group(1)] = int(m.group(2))
    return body, meta


def counts(ins):
    op = [i.split()[0] for i in ins]
    is_mfma = [o.startswith("v_mfma") or o.startswith("v_smfmac") for o in op]
    gload = [o.startswith("global_load") for o in op]
    serial = sum(1 for k in range(len(ins) - 1) if gload[k] and op[k + 1] == "s_waitcnt" and "vmcnt(0)" in ins[k + 1])
    pos = [k for k, f in enumerate(is_mfma) if f]
    head = pos[0] if pos else len(ins)
    tail = len(ins) - 1 - pos[-1] if pos else 0
    gap = max((b - a - 1 for a, b in zip(pos, pos[1:])), default=0)
    return {"insts": len(ins), "mfma": len(pos), "gload": sum(gload), "gstore": sum(o.startswith("global_store") for o in op),
            "serial": serial, "scratch_ld": sum(o.startswith("scratch_load") for o in op),
            "scratch_st": sum(o.startswith("scratch_store") for o in op), "head": head, "gap": gap, "tail": tail}


def main():
    path = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "nerfmlp_dgrad_kernel"
    body, meta = kernels(path)
    names = sorted(body)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    print("| kernel | insts | mfma | gload | gstore | serial | scratch ld/st | head | gap | tail | spill | priv |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for n, d in zip(names, dem):
        if want not in d or not body[n]:
            continue
        c, m = counts(body[n]), meta.get(n, {})
        short = re.sub(r"^void rnerf::|\(.*$", "", d)
        print(f"| `{short}` | {c['insts']} | {c['mfma']} | {c['gload']} | {c['gstore']} | {c['serial']} | {c['scratch_ld']}/{c['scratch_st']} | "
              f"{c['head']} | {c['gap']} | {c['tail']} | {m.get('vgpr_spill_count', '?')} | {m.get('private_segment_fixed_size', '?')} |")


if __name__ == "__main__":
    main()
