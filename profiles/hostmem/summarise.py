"""Per-figure table of one session directory: python session.py DIR"""
import collections, glob, json, os, sys
d = sys.argv[1]
def load(pattern):
    fig, order = collections.OrderedDict(), []
    for f in sorted(glob.glob(os.path.join(d, pattern))):
        tag = os.path.basename(f).split('seq')[1].split('.')[0]
        order.append(tag)
        for l in open(f):
            if l.startswith('{'):
                r = json.loads(l)
                if 'ms_per_step' in r:
                    fig.setdefault(f"{r['kind']} {r['path']}", {})[tag] = r['ms_per_step'] * 1e3
    return fig, order
total = bad = 0
for pattern, title in (('emtrain_ens_time_seq*.jsonl', 'sp0, sp1, tp'), ('emtrain_ens_time_ms_seq*.jsonl', 'ms0, ms1')):
    fig, order = load(pattern)
    print(f"emtrain_ens_time.py --K 1, kinds {title}: us per step, lower is better; runs in order:")
    print("  " + " ".join(order))
    print("  a round is (parent, X, parent), X = new or control (a second copy of the parent tree);")
    print("  excess = X - max(its two parents); allowed = the largest gap between consecutive parent runs")
    print(f"  {'figure':9s} {'parent mean':>11s} {'new mean':>9s} {'allowed':>8s}  new excess per round      control excess per round   new ok")
    for n, v in fig.items():
        vals = [v[t] for t in order]
        par = [i for i, t in enumerate(order) if 'parent' in t]
        gaps = [abs(vals[a] - vals[b]) for a, b in zip(par, par[1:])]
        ex = lambda kind: [vals[i] - max(vals[i - 1], vals[i + 1]) for i, t in enumerate(order) if kind in t]
        en, ec = ex('new'), ex('control')
        ok = round(max(en), 2) <= round(max(gaps), 2)   # the tool prints 0.01 us steps
        total += 1
        bad += not ok
        mean = lambda kind: sum(vals[i] for i, t in enumerate(order) if kind in t) / sum(kind in t for t in order)
        print(f"  {n:9s} {mean('parent'):11.2f} {mean('new'):9.2f} {max(gaps):8.2f}  " + " ".join(f"{x:+7.2f}" for x in en) +
              "    " + " ".join(f"{x:+7.2f}" for x in ec) + f"    {'yes' if ok else 'NO'}")
print(f"new figures outside the parent's spread: {bad} of {total}")
