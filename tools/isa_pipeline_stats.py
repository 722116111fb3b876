"""Development only: how far ahead of their use the GEMM passes of k_encoder_fused<RTT> request their operands, read off
the ISA listing (the static check recorded in profiles/README.md).

    hipcc <flags of eam_rl4co_amd/build.py> -S --cuda-device-only eam_rl4co_amd/csrc/encoder_fused.hip -o enc.s
    python tools/isa_pipeline_stats.py enc.s

The kernel body is walked in program order (branches ignored).  Outstanding LDS reads and global loads are kept in two queues
the way the hardware counters work (both return in order): `s_waitcnt lgkmcnt(N)` / `vmcnt(N)` retires all but the newest N,
and every retired load is booked with the number of MFMAs issued between it and that wait.  "In-pass" weight loads are the
global_load_dwordx4 with an MFMA among the 12 instructions before AND after them (the first fragments of a pass are issued
outside the MFMA stream).
"""
import re
import sys
from collections import Counter


def main(path):
    src = open(path).read().split("\n")
    for rtt in (2, 4, 7):
        name = f"_ZN5eamrl15k_encoder_fusedILi{rtt}EEEvNS_9FusedArgsE"
        cand = [i for i, l in enumerate(src) if l.startswith(name + ":")]
        if not cand:
            continue
        s = cand[0]
        e = next(i for i in range(s, len(src)) if src[i].strip().startswith("s_endpgm"))
        body = [l.strip().split(";")[0].strip() for l in src[s + 1:e]]
        body = [l for l in body if l and not l.startswith(".") and not l.endswith(":")]
        meta = {}
        for l in src[e:]:
            m = re.match(r"\s*;\s*(NumVgprs|ScratchSize|Occupancy):\s*(\d+)", l)
            if m and m.group(1) not in meta:
                meta[m.group(1)] = int(m.group(2))
            if len(meta) == 3:
                break
        ops = [l.split()[0] for l in body]
        is_mfma = [o.startswith("v_mfma") for o in ops]
        nm = 0
        lq, vq = [], []             # outstanding LDS reads / global loads: (MFMA index at issue, in-pass weight load?)
        ldist, vdist = [], []
        nwait = imm = 0
        for k, (ins, op) in enumerate(zip(body, ops)):
            if is_mfma[k]:
                nm += 1
            elif op.startswith("ds_read"):
                lq.append(nm)
            elif op.startswith(("global_load", "flat_load")):
                inpass = op.endswith("dwordx4") and any(is_mfma[max(0, k - 12):k]) and any(is_mfma[k + 1:k + 13])
                vq.append((nm, inpass))
            elif op == "s_waitcnt":
                nwait += 1
                m = re.search(r"lgkmcnt\((\d+)\)", ins)
                if m:
                    n = int(m.group(1))
                    if n == 0 and k and ops[k - 1].startswith("ds_read"):
                        imm += 1
                    r = len(lq) - n
                    if r > 0:
                        ldist += [nm - x for x in lq[:r]]
                        lq = lq[r:]
                m = re.search(r"vmcnt\((\d+)\)", ins)
                if m:
                    n = int(m.group(1))
                    r = len(vq) - n
                    if r > 0:
                        vdist += [(nm - x, p) for x, p in vq[:r]]
                        vq = vq[r:]
        inp = [d for d, p in vdist if p]
        print(f"RTT={rtt}: VGPRs {meta.get('NumVgprs')}, scratch {meta.get('ScratchSize')} B, MFMA {sum(is_mfma)}, s_waitcnt {nwait}, "
              f"LDS reads {len(ldist)}")
        print(f"   LDS reads directly followed by lgkmcnt(0): {imm};  waited on with no MFMA in between: {sum(d == 0 for d in ldist)};  "
              f"with >= 16 MFMAs in between: {sum(d >= 16 for d in ldist)}")
        print(f"   in-pass weight loads: {len(inp)}, MFMAs between load and wait: min {min(inp) if inp else '-'}, "
              f"histogram {sorted(Counter(inp).items())}")


if __name__ == "__main__":
    main(sys.argv[1])
