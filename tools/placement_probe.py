#!/usr/bin/env python3
"""Runs tools/placement_probe (a launch shaped like k_combine_fast<Fq2>'s whose waves record where and when they ran) and
answers the question DESIGN.md 5.2 needs answered before a launch ORDER can pair waves: with R resident waves, is the wave that
shares a SIMD with workgroup k a fixed function of k?

  python tools/placement_probe.py [--hold-us 200] [--repeats 3] [--grids 2296 2048 4592] [--map-out FILE] [--records FILE]

Reports per launch
  * the share of workgroups k < R/2 for which workgroup k + R/2 started on the same SIMD while k was resident;
  * the differences (partner - k) seen among the first R workgroups, most frequent first, and whether the partner map is
    the same in every repeat;
  * where the workgroups past R go (the SIMD that frees a seat first, or a fixed one).
--map-out writes the partner of every k as JSON ({"resident": R, "partner": [...]} for the first launch, and the same per
launch under "launches"), the form tools/sim_launch_order.py --placement reads.  --records analyses a saved output of the program instead of running it."""
import argparse
import collections
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def run_probe(hold_us, repeats, grids, timeout):
    exe = os.path.join(HERE, "placement_probe")
    if not os.path.exists(exe):
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", os.path.join(HERE, "placement_probe.hip"), "-o", exe], check=True)
    # ONE time limit for the whole program: its launches end by the clock, whatever the placement
    out = subprocess.run([exe, str(hold_us), str(repeats)] + [str(g) for g in grids], check=True, capture_output=True, text=True, timeout=timeout)
    return out.stdout


def parse(text):
    head, launches = {}, collections.OrderedDict()
    for line in text.splitlines():
        if line.startswith("#"):
            w = line[1:].split()
            head = {w[i]: w[i + 1] for i in range(0, len(w) - 1, 2)}
            continue
        f = line.split()
        if len(f) != 10:
            continue
        g, r, b, xcc, se, cu, simd, slot, t0, t1 = (int(x) for x in f)
        launches.setdefault((g, r), {})[b] = {"simd": (xcc, se, cu, simd), "slot": slot, "start": t0, "end": t1}
    return head, launches


def partner_map(recs, R):
    """partner[k] for k < R: the other workgroup of the first R that sat on k's SIMD while k was resident (-1: none or several)"""
    by_simd = collections.defaultdict(list)
    for k in range(min(R, len(recs))):
        by_simd[recs[k]["simd"]].append(k)
    partner = [-1] * R
    for ks in by_simd.values():
        for k in ks:
            over = [j for j in ks if j != k and recs[j]["start"] < recs[k]["end"] and recs[k]["start"] < recs[j]["end"]]
            if len(over) == 1:
                partner[k] = over[0]
    return partner, by_simd


def analyse(head, launches, map_out=None):
    R = int(head.get("resident", 0))
    lines = ["device %s  CUs %s  workgroups per CU %s  resident R = %d  hold %s us" % (head.get("device"), head.get("cus"), head.get("workgroups_per_cu"), R, head.get("hold_us"))]
    first_map, maps = None, {}
    for (g, r), recs in launches.items():
        partner, by_simd = partner_map(recs, R)
        half = R // 2
        hit = sum(1 for k in range(half) if partner[k] == k + half)
        seats = collections.Counter(len(v) for v in by_simd.values())
        diffs = collections.Counter(partner[k] - k for k in range(R) if partner[k] > k)
        unpaired = sum(1 for k in range(min(R, g)) if partner[k] < 0)
        first_round_start = max(recs[k]["start"] for k in range(min(R, g)))
        lines.append("grid %d repeat %d: SIMDs used by the first R %d, first-R workgroups per SIMD %s, last first-round start %.1f us" %
                     (g, r, len(by_simd), dict(sorted(seats.items())), first_round_start / 100.0))
        lines.append("  k + R/2 on the same SIMD while k resident: %d of %d = %.3f   (first-R workgroups with no single partner: %d)" % (hit, half, hit / max(half, 1), unpaired))
        lines.append("  partner - k, most frequent: %s" % ", ".join("%+d x%d" % (d, c) for d, c in diffs.most_common(8)))
        # the same question inside an XCC: workgroups go to the XCCs round robin, so the index that matters may be k div #XCC
        nx = len({s[0] for s in by_simd})
        xdiffs = collections.Counter((partner[k] // nx) - (k // nx) for k in range(R) if partner[k] > k and recs[k]["simd"][0] == k % nx)
        xcc_rr = sum(1 for k in range(min(R, g)) if recs[k]["simd"][0] == k % nx)
        lines.append("  XCCs %d; workgroup k on XCC k mod %d: %d of %d; partner - k in units of the XCC's own sequence: %s" %
                     (nx, nx, xcc_rr, min(R, g), ", ".join("%+d x%d" % (d, c) for d, c in xdiffs.most_common(6))))
        if g > R:
            # a surplus workgroup takes the seat of the first-round workgroup that ended just before it started
            took = collections.Counter()
            for b in range(R, g):
                prev = [k for k in by_simd.get(recs[b]["simd"], []) if recs[k]["end"] <= recs[b]["start"]]
                took["seat of a finished first-round workgroup" if prev else "other"] += 1
            order_ok = sum(1 for b in range(R, g - 1) if recs[b]["start"] <= recs[b + 1]["start"])
            lines.append("  surplus %d: %s; started in index order: %d of %d" % (g - R, dict(took), order_ok, g - R - 1))
        maps.setdefault(g, []).append(partner)
        if first_map is None:
            first_map = partner
    for g, ms in maps.items():
        same = sum(1 for m in ms[1:] if m == ms[0])
        agree = [sum(1 for a, b in zip(ms[0], m) if a == b) / max(len(m), 1) for m in ms[1:]]
        lines.append("grid %d: partner map identical to repeat 0 in %d of %d repeats; share of equal entries %s" % (g, same, len(ms) - 1, ["%.3f" % a for a in agree]))
    if map_out and first_map is not None:
        # the first launch's map at the top level, every launch's under "launches" (tools/sim_launch_order.py --placement reads both)
        with open(map_out, "w") as f:
            json.dump({"resident": R, "partner": first_map,
                       "launches": [{"grid": g, "repeat": r, "partner": m} for g, ms in maps.items() for r, m in enumerate(ms)]}, f)
    return "\n".join(lines)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--hold-us", type=float, default=200.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--grids", type=int, nargs="*", default=[2296, 2048, 4592])
    ap.add_argument("--timeout", type=float, default=60.0)
    ap.add_argument("--map-out")
    ap.add_argument("--records")
    ap.add_argument("--save-records")
    a = ap.parse_args()
    text = open(a.records).read() if a.records else run_probe(a.hold_us, a.repeats, a.grids, a.timeout)
    if a.save_records:
        with open(a.save_records, "w") as f:
            f.write(text)
    head, launches = parse(text)
    if not launches:
        sys.exit("no records")
    print(analyse(head, launches, a.map_out))
