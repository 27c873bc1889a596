"""Summary of recipes/ab_parent.sh: per leg the three parent and three new figures, medians, the parent's spread and the
rules of profiles/scan128/README.md; the forward scan's ms per launch (roofline.avg_kernel_ms) of the headline runs."""
import json, sys, os, statistics
d, out = sys.argv[1], sys.argv[2]
def last_json(p):
    if not os.path.exists(p): return None
    for line in reversed(open(p).read().strip().split("\n")):
        line = line.strip()
        if line.startswith("{"):
            try: return json.loads(line)
            except Exception: pass
    return None
def leg_ms(j, leg):
    if leg in ("headline", "headline_of_the_full_runs"): return j.get("ms_per_step")
    if leg == "scan_ms_per_launch": return (j.get("roofline") or {}).get("avg_kernel_ms")
    v = j.get(leg)
    if not isinstance(v, dict): return None
    for k in ("ms_per_step", "ms_per_call", "ms"):
        if k in v: return v[k]
    return None
res = {
    "cmd": ["python bench.py --gpus 1 --steps 20 --warmup 5", "python bench.py --full --no-db --no-config3 --no-config4"],
    "how": "one GPU call (profiles/scan128/recipes/ab_parent.sh), alternating parent1 / new1 / parent2 / new2 / parent3 / new3; parent = the parent commit's library (tools/ab_prev_lib.sh) selected with AMC_LIB_PATH, new = the tree's own library; each step under its own timeout, chained with &&.  The db leg is left out: it goes through the host module, which links libamc.so directly and cannot be switched this way.",
    "rule": "headline: the new median must be below the parent's median by more than three times the parent's max - min of this call (gain_over_three_spreads).  Every other leg: the new median may exceed the parent's median by at most the parent's max - min (within_parent_spread).",
    "ms_per_step": {}, "summary": {}, "other": {}}
runs = {}
for kind in ("head", "full"):
    for who in ("parent", "new"):
        for i in (1, 2, 3):
            runs[(kind, who, i)] = last_json(f"{d}/{kind}_{who}{i}.json")
legs = [("headline", "head"), ("scan_ms_per_launch", "head")]
legs += [(l, "full") for l in ("headline_of_the_full_runs", "verify", "pipeline", "dense", "ragged", "sift_stats")]
for leg, kind in legs:
    vals = {}
    for who in ("parent", "new"):
        for i in (1, 2, 3):
            j = runs[(kind, who, i)]
            if j is not None:
                v = leg_ms(j, leg)
                if v is not None: vals[f"{who}{i}"] = round(float(v), 3)
    res["ms_per_step"][leg] = vals
    p = [vals[k] for k in vals if k.startswith("parent")]
    n = [vals[k] for k in vals if k.startswith("new")]
    if len(p) == 3 and len(n) == 3:
        pm, nm, sp = statistics.median(p), statistics.median(n), max(p) - min(p)
        res["summary"][leg] = {"parent_median": pm, "new_median": nm, "parent_spread": round(sp, 3),
                               "new_minus_parent": round(nm - pm, 3), "within_parent_spread": nm - pm <= sp,
                               "gain_over_three_spreads": pm - nm > 3 * sp}
for (kind, who, i), j in runs.items():
    if j is None or kind != "full": continue
    o = {}
    for leg in ("ragged", "sift_stats", "dense", "pipeline", "verify", "cpu_baseline"):
        v = j.get(leg)
        if isinstance(v, dict):
            o[leg] = {k: v[k] for k in ("vs_uniform", "gpu_vs_oracle_mismatching_pairs", "value") if k in v}
    res["other"][f"{who}{i}"] = o
json.dump(res, open(out, "w"), indent=1)
print(json.dumps(res["summary"], indent=1))
print(json.dumps(res["other"]))
