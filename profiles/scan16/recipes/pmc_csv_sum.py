import csv, sys, collections
acc = collections.defaultdict(lambda: [0, 0.0])
with open(sys.argv[1]) as f:
    for r in csv.DictReader(f):
        k = (r["Kernel_Name"][:90], r["Counter_Name"])
        acc[k][0] += 1
        acc[k][1] += float(r["Counter_Value"])
flt = sys.argv[2] if len(sys.argv) > 2 else ""
for (kn, cn), (n, s) in sorted(acc.items()):
    if flt in kn:
        print(f"{kn:90s} {cn:28s} n={n:<5d} sum={s:.6g} avg={s / n:.6g}")
