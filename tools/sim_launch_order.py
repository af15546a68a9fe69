#!/usr/bin/env python3
"""When does the headline G2 combine launch end under a given ORDER of its waves?  A CPU model, not a measurement.

Rules
  * 1024 SIMDs with two seats each (R = 2048 resident waves; --simds changes it).
  * Two waves that share a SIMD each advance at 2/3 of a lone wave's speed: waves of lone cost a >= b that start together end
    at 1.5 b and a + 0.5 b.
  * Workgroups are dispatched in index order into free seats, one per SIMD before any SIMD gets a second: wave k < R/2 sits
    beside wave k + R/2.  --placement FILE replaces that by a measured map (tools/placement_probe.py --map-out:
    {"resident": R, "partner": [...]}); waves past R take the seat that frees first.
  * The cost of a wave is its subset's multiply-adds per job in profiles/combine_uniform_macs.json (uniform_v_mad), in units
    of W = the mean of the generic subsets.

  python tools/sim_launch_order.py                       # the table of orders at 65 536, 131 072 and 262 144 jobs
  python tools/sim_launch_order.py --jobs 65536 --seed 3
  python tools/sim_launch_order.py --counts counts.json  # {"0 1 2 3": 312, ...} jobs per subset instead of a draw
  python tools/sim_launch_order.py --cost-file other.json  # another cost per subset (same layout), e.g. a prediction
  python tools/sim_launch_order.py --sweep 64000 70000 76000   # where the fold stops paying (the 19/16 bound)
  python tools/sim_launch_order.py --placement profiles/placement_maps.json --every-launch --jobs 65536

Orders: present (generic groups in table order, then 2^a, then D = 1), descending, aligned (heaviest R/2 descending; of the
rest the cheapest surplus last, the others ascending behind slot R/2 so that each sits beside the heavy wave of its rank),
packed (explicit longest-first packing onto seats: what any order could reach at best), and the fluid bound."""
import argparse
import heapq
import json
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))
MACS = os.path.join(HERE, "..", "profiles", "combine_uniform_macs.json")
PAIRED = 2.0 / 3.0
WAVE_JOBS = 32


def load_costs(path=MACS, field="uniform_v_mad"):
    d = json.load(open(path))
    subsets = d["subsets"]
    generic = [v[field] for v in subsets.values() if cls_of(v["D"]) == 0]
    unit = sum(generic) / len(generic)
    return {k: {"D": v["D"], "cost": v[field] / unit, "cls": cls_of(v["D"])} for k, v in subsets.items()}, unit


def cls_of(D):
    """0 generic, 1 a power of two, 2 D = 1 (the order of k_combine_plan's classes)"""
    D = abs(D)
    if D == 1:
        return 2
    return 1 if D & (D - 1) == 0 and D <= 1 << 16 else 0


def table_entry(subset):
    """where the call's table keeps the subset's key (tc_jobs.h combine_key_hash / combine_probe_step, before collisions)"""
    key = 0
    for k, i in enumerate(int(x) for x in subset.split()):
        key |= i << (16 * k)
    h = ((key * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> 40
    return h & 511


def draw_counts(subsets, jobs, seed):
    rng = random.Random(seed)
    names = sorted(subsets)
    counts = dict.fromkeys(names, 0)
    for _ in range(jobs):
        counts[names[rng.randrange(len(names))]] += 1
    return counts


def waves_of(counts, subsets):
    """one entry per wave: (cost, class, subset)"""
    out = []
    for name, n in counts.items():
        out += [(subsets[name]["cost"], subsets[name]["cls"], name)] * ((n + WAVE_JOBS - 1) // WAVE_JOBS)
    return out


def default_partner(R):
    return [k + R // 2 if k < R // 2 else k - R // 2 for k in range(R)]


def order_present(waves):
    return sorted(waves, key=lambda w: (w[1], table_entry(w[2]), w[2]))


def order_descending(waves):
    return sorted(waves, key=lambda w: (-w[0], w[2]))


def order_aligned(waves, R, partner=None):
    """heaviest R/2 descending in the first seats; of the rest the cheapest max(0, rest - R/2) last, the others ascending in
    the second seats, the i-th lightest beside the i-th heaviest (through the partner map)"""
    partner = partner or default_partner(R)
    desc = order_descending(waves)
    half = R // 2
    if len(desc) < R:
        return desc
    firsts = [k for k in range(R) if partner[k] > k] if all(p >= 0 for p in partner) else list(range(half))
    if len(firsts) != half:
        firsts = list(range(half))
    head, rest = desc[:half], desc[half:]
    surplus = len(rest) - half
    beside = rest[:half]                       # still descending: beside[-1] is the lightest that stays in the round
    last = rest[half:]
    slots = [None] * R
    # heavy wave of rank i takes the i-th first seat; the lightest kept wave goes beside rank 0
    for i, k in enumerate(firsts):
        slots[k] = head[i]
        slots[partner[k]] = beside[half - 1 - i]
    assert surplus == len(last) and all(s is not None for s in slots)
    return slots + last


def makespan(order, R, partner=None):
    """event simulation: the first R waves take their seats at t = 0 (wave k beside partner[k]); every later wave takes the
    seat that frees first, in index order"""
    partner = partner or default_partner(R)
    simd_of, nsimd = {}, 0
    for k in range(R):
        if k in simd_of:
            continue
        simd_of[k] = nsimd
        p = partner[k]
        if 0 <= p < R and p not in simd_of:
            simd_of[p] = nsimd
        nsimd += 1
    seats = [[] for _ in range(nsimd)]          # remaining lone cost per resident wave
    clock = [0.0] * nsimd
    first = min(len(order), R)
    for k in range(first):
        seats[simd_of[k]].append(order[k][0])
    nxt = first
    heap = []

    def push(i):
        if seats[i]:
            rate = PAIRED if len(seats[i]) > 1 else 1.0
            heapq.heappush(heap, (clock[i] + min(seats[i]) / rate, i, len(seats[i]), min(seats[i])))

    for i in range(nsimd):
        push(i)
    end = 0.0
    while heap:
        t, i, n, m = heapq.heappop(heap)
        if n != len(seats[i]) or not seats[i] or m != min(seats[i]):
            continue                            # a stale event
        rate = PAIRED if n > 1 else 1.0
        done = (t - clock[i]) * rate
        seats[i] = [r - done for r in seats[i]]
        clock[i] = t
        seats[i].remove(min(seats[i]))
        end = max(end, t)
        if nxt < len(order):
            seats[i].append(order[nxt][0])
            nxt += 1
        push(i)
    return end


def simd_end(a, b):
    """two seats that each run their waves one after the other, started together"""
    qa, qb = list(a), list(b)
    ra, rb = (qa.pop(0) if qa else None), (qb.pop(0) if qb else None)
    t = 0.0
    while ra is not None or rb is not None:
        if ra is not None and rb is not None:
            d = min(ra, rb)
            t += d / PAIRED
            ra, rb = ra - d, rb - d
        else:
            t += ra if ra is not None else rb
            ra = rb = 0.0
        if ra is not None and ra <= 1e-12:
            ra = qa.pop(0) if qa else None
        if rb is not None and rb <= 1e-12:
            rb = qb.pop(0) if qb else None
    return t


def makespan_packed(waves, R):
    """explicit longest-first packing: every wave, heaviest first, goes to the (SIMD, seat) that then ends earliest"""
    nsimd = R // 2
    q = [([], []) for _ in range(nsimd)]
    heap = [(0.0, i) for i in range(nsimd)]
    heapq.heapify(heap)
    for w in order_descending(waves):
        _, i = heapq.heappop(heap)
        a, b = q[i]
        ea, eb = simd_end(a + [w[0]], b), simd_end(a, b + [w[0]])
        if ea <= eb:
            a.append(w[0])
        else:
            b.append(w[0])
        heapq.heappush(heap, (min(ea, eb), i))
    return max(e for e, _ in heap)


def aligned_applies(n_waves, R, bound=19 / 16):  # tc_jobs.h combine_order_aligned
    return R <= n_waves <= bound * R


def report(jobs, subsets, R, partner, seed, counts=None):
    counts = counts or draw_counts(subsets, jobs, seed)
    waves = waves_of(counts, subsets)
    work = sum(w[0] for w in waves)
    rows = [("present (generic in table order, 2^a, 1)", makespan(order_present(waves), R, partner)),
            ("all waves by descending cost", makespan(order_descending(waves), R, partner)),
            ("aligned (heaviest R/2 descending, rest ascending beside them, cheapest surplus last)", makespan(order_aligned(waves, R, partner), R, partner)),
            ("explicit longest-first packing onto seats", makespan_packed(waves, R)),
            ("fluid bound: work / (SIMDs x 1.333)", work / ((R // 2) * 2 * PAIRED))]
    ncls = [sum(1 for w in waves if w[1] == c) for c in range(3)]
    out = ["jobs %d: waves %d (generic %d, 2^a %d, D=1 %d), R %d, work %.1f W, aligned regime %s" %
           (sum(counts.values()), len(waves), ncls[0], ncls[1], ncls[2], R, work, "applies" if aligned_applies(len(waves), R) else "does not apply (descending is used)")]
    for name, t in rows:
        out.append("  %-88s %.3f W" % (name, t))
    return "\n".join(out), dict(rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, nargs="*", default=[65536, 131072, 262144])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--simds", type=int, default=1024)
    ap.add_argument("--counts")
    ap.add_argument("--sweep", type=int, nargs="*", help="batch sizes: descending against folded at each")
    ap.add_argument("--every-launch", action="store_true", help="with --placement: the orders under each recorded launch's map")
    ap.add_argument("--placement")
    ap.add_argument("--cost-file", default=MACS)
    ap.add_argument("--cost-field", default="uniform_v_mad")
    a = ap.parse_args()
    subsets, unit = load_costs(a.cost_file, a.cost_field)
    R, partner, launches = 2 * a.simds, None, None
    if a.placement:
        m = json.load(open(a.placement))
        R, partner = m["resident"], m["partner"]
        if a.every_launch:
            R, partner, launches = m["resident"], None, m["launches"]
    print("model: %d SIMDs x 2 seats, paired waves at %.3f each; W = %.0f multiply-adds per job (mean of the generic subsets)%s" %
          (R // 2, PAIRED, unit, "; placement map from " + os.path.basename(a.placement) if partner else "; wave k beside wave k + R/2"))
    if a.sweep:
        # where the fold stops paying: waves / R against the two orders (the bound of tc_jobs.h combine_order_aligned)
        print("sweep: jobs, waves / R, descending, folded (W)")
        for jobs in a.sweep:
            w = waves_of(draw_counts(subsets, jobs, a.seed), subsets)
            folded = "%.3f" % makespan(order_aligned(w, R, partner), R, partner) if len(w) >= R else "  -  "
            print("  %7d  %.3f  %.3f  %s" % (jobs, len(w) / R, makespan(order_descending(w), R, partner), folded))
    elif launches:
        # orders built for k <-> k + R/2, run under the measured partner of every k, launch by launch
        w = waves_of(draw_counts(subsets, a.jobs[0], a.seed), subsets)
        print("jobs %d under every measured launch: grid, repeat, share of k beside k + R/2, present, descending, folded (W)" % a.jobs[0])
        for m in launches:
            pm = m["partner"]
            share = sum(1 for k in range(R // 2) if pm[k] == k + R // 2) / (R // 2)
            print("  %5d #%d  %.3f  %.3f  %.3f  %.3f" % (m["grid"], m["repeat"], share, makespan(order_present(w), R, pm),
                                                        makespan(order_descending(w), R, pm), makespan(order_aligned(w, R), R, pm)))
    elif a.counts:
        print(report(0, subsets, R, partner, a.seed, json.load(open(a.counts)))[0])
    else:
        for jobs in a.jobs:
            print(report(jobs, subsets, R, partner, a.seed)[0])
