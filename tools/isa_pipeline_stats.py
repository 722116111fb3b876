"""Development only: how far ahead of their use the GEMM passes of k_encoder_fused<RTT> request their operands, read off
the ISA listing (the static check recorded in profiles/README.md).

    hipcc <flags of eam_rl4co_amd/build.py> -S --cuda-device-only eam_rl4co_amd/csrc/encoder_fused.hip -o enc.s
    python tools/isa_pipeline_stats.py enc.s

The kernel body is walked in program order (branches ignored).  Outstanding LDS reads and global loads are kept in two queues
the way the hardware counters work (both return in order): `s_waitcnt lgkmcnt(N)` / `vmcnt(N)` retires all but the newest N,
and every retired load is booked with the number of MFMAs issued between it and that wait.  "In-pass" weight loads are the
global_load_dwordx4 with an MFMA among the 12 instructions before AND after them (the first fragments of a pass are issued
outside the MFMA stream).

For the stages around the GEMM passes (init embedding / load of h, constants staging, graph context, cache passes) the
listing is cut into load -> LDS-store episodes (`episodes`, `prologue_stats`): what matters there is how many batches of loads
wait for one another between a stage's first load and its last LDS store, and whether a pointer is itself fetched by a vector
load.  The walk is in program order: it does not know trip counts (an episode inside a loop is marked), and the episodes of
the layer loop also pick up the GEMM passes' own weight loads.
"""
import re
import sys
from collections import Counter


def vmc(ins):
    return int(re.search(r"vmcnt\((\d+)\)", ins).group(1))


def episodes(body, ops, lo, hi):
    """The load -> LDS-store episodes of body[lo:hi] (labels kept, as their own entries): an episode runs from a global load to
    the last ds_write before the next global load or barrier that follows a ds_write.  Per episode: its first instruction, the loads by
    width, the vmcnt waits up to the last ds_write with their counts, round trips = 1 + the waits that have a load of the
    episode behind them (batches of loads that wait for one another), and whether a branch ahead of its last ds_write goes back
    to a label inside it (then all of this is per loop trip)."""
    out, cur = [], None
    for k in range(lo, hi):
        op = ops[k]
        if op.startswith("global_load"):
            if cur is None or cur["stored"]:
                if cur is not None:
                    out.append(cur)
                cur = {"at": k, "loads": Counter(), "ev": [], "stored": False, "labels": set(), "loop": False}
            cur["loads"][op.replace("global_load_", "")] += 1
            cur["ev"].append("L")
        elif cur is None:
            continue
        elif op == "s_barrier" and cur["stored"]:       # stores behind a later barrier belong to another stage
            out.append(cur)
            cur = None
        elif op.endswith(":"):
            cur["labels"].add(op[:-1])
        elif op.startswith(("s_cbranch", "s_branch")) and body[k].split()[-1] in cur["labels"]:
            cur["ev"].append("B")
        elif op == "s_waitcnt" and "vmcnt" in body[k]:
            cur["ev"].append(vmc(body[k]))
        elif op.startswith("ds_write"):
            cur["stored"] = True
            cur["ev"].append("S")
    if cur is not None and cur["stored"]:
        out.append(cur)
    for e in out:
        ev = e["ev"][:len(e["ev"]) - e["ev"][::-1].index("S")]
        e["loop"] = "B" in ev
        e["waits"] = [x for x in ev if isinstance(x, int)]
        e["trips"] = 1 + sum(1 for i, x in enumerate(ev) if isinstance(x, int) and "L" in ev[i + 1:])
    return out


def vector_pointer_fetches(body, ops):
    """global_load_dwordx2 whose result is the address of a later global load (a pointer fetched through the vector path)"""
    n, regs = 0, set()
    for k in range(len(ops)):
        if not ops[k].startswith("global_load"):
            continue
        args = body[k].split(None, 1)[1].split(",")
        if len(args) > 1 and args[1].strip().split()[0] in regs:
            n += 1
        if ops[k] == "global_load_dwordx2":
            regs.add(args[0].strip())
    return n


def prologue_stats(body, ops):
    """The stages around the GEMM passes (body with its labels).  Init embedding and constants staging are the episodes whose
    loads are 32 bits wide (the weights of the GEMM passes come as dwordx4), reported with the number of workgroup barriers
    in front of them: 0 = init embedding / load of h, 1 or more = inside the layer loop.  The graph context ends at the only
    global_store_dword and starts two barriers before it; the cache passes follow."""
    bars = [k for k, o in enumerate(ops) if o == "s_barrier"]
    g = [k for k, o in enumerate(ops) if o == "global_store_dword"]
    end = [b for b in bars if b < g[0]][-2] if g else len(ops)
    print("   load -> LDS-store episodes ahead of the graph context (kernel entry: h or the init embedding, one per path; layer loop):")
    for e in episodes(body, ops, 0, end):
        if e["at"] > bars[0] and set(e["loads"]) == {"dwordx4"}:
            continue            # first weights of a GEMM pass followed by its epilogue's stores
        print(f"      barriers ahead {sum(b < e['at'] for b in bars)}: loads {dict(e['loads'])}, vmcnt waits {e['waits']}, round trips "
              f"{e['trips']}{' PER TRIP OF A LOOP' if e['loop'] else ''}")
    w = [vmc(body[k]) for k in range(bars[0], bars[1]) if ops[k] == "s_waitcnt" and "vmcnt" in body[k]]
    print(f"   vmcnt waits between the first two barriers in program order: {w}")
    print(f"   pointers fetched by vector loads (whole kernel): {vector_pointer_fetches(body, ops)}")
    if g:
        ld = [k for k in range(end, g[0]) if ops[k].startswith("global_load")]
        w = [k for k in range(ld[0], g[0]) if ops[k] == "s_waitcnt" and "vmcnt" in body[k]] if ld else []
        mid = [b for b in bars if b < g[0]][-1]
        print(f"   graph context: {len(ld)} loads, {sum(k < mid for k in ld)} of them ahead of the mean's barrier, "
              f"vmcnt waits {[vmc(body[k]) for k in w]}")
        early = 0
        stores = [k for k in range(g[0], len(ops)) if ops[k] == "global_store_dwordx4"]
        mf = [k for k in range(g[0], len(ops)) if ops[k].startswith("v_mfma")]
        for s in stores:
            prev = [k for k in mf if k < s]
            if prev and not any(ops[k] == "global_store_dwordx4" for k in range(prev[-1], s)):
                early += sum(ops[k] == "global_load_dwordx4" for k in range(prev[-1], s))
        print(f"   cache passes: first-weight loads issued between a pass's last MFMA and its first global store: {early}")


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
        lbody = [l.strip().split(";")[0].strip() for l in src[s + 1:e]]
        lbody = [l for l in lbody if l and (not l.startswith(".") or l.startswith(".LBB"))]
        prologue_stats(lbody, [l.split()[0] for l in lbody])


if __name__ == "__main__":
    main(sys.argv[1])
