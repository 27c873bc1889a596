"""One line per run of recipes/pick_run.sh: file, ms per step, the forward scan's ms per launch, matches."""
import glob, json, os, sys
for f in sorted(glob.glob(os.path.join(sys.argv[1], "*.json"))):
    j = [json.loads(l) for l in open(f) if l.startswith("{")][-1]
    print(os.path.basename(f), j["ms_per_step"], j["roofline"]["avg_kernel_ms"], j["config"]["matches_rank0"])
