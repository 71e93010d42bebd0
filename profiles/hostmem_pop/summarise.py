"""Per-figure table of the parent / new runs in this directory: python summarise.py [DIR]

Runs are <tool>_parent<r>.txt and <tool>_new<r>.txt, r = 1..3, taken in the order parent1, new1,
parent2, new2, parent3, new3.  Criterion per figure: new's worst run is not worse than the
parent's worst run by more than the largest gap between consecutive parent runs."""
import collections, glob, json, os, statistics, sys

d = sys.argv[1] if len(sys.argv) > 1 else os.path.dirname(os.path.abspath(__file__))


def records(path):
    text = open(path).read().strip()
    if text.startswith("["):
        return json.loads(text)
    return [json.loads(l) for l in text.splitlines() if l.startswith("{")]


def figures(tool, recs):
    """{figure: (value, higher_is_better)} of one run."""
    out = collections.OrderedDict()
    if tool == "bench":
        r = recs[-1]
        out["member-grad-steps/s"] = (r["value"], True)
        if r.get("eval_rollout"):
            out["eval rollout ms"] = (r["eval_rollout"]["ms"], False)
    elif tool == "ens_time":
        s = [r for r in recs if r.get("summary")][-1]
        for k in ("loop_ms", "per_model_ms", "single_ms", "mixed_ms"):
            out[k] = (s[k], False)
    elif tool == "em_replay_time":
        by = collections.defaultdict(list)
        for r in recs:
            if "wall_ms" in r:
                by[f"{r['shape']} n={r['n']} wall_ms (median)"].append(r["wall_ms"])
        for k, v in by.items():
            out[k] = (statistics.median(v), False)
    else:  # synth_time, pbt_time
        for r in recs:
            what = r.get("what")
            if what == "step_rate":
                out[f"step_rate rho={r['real_ratio']} member-steps/s"] = (r["median"], True)
            elif what == "tune":
                out[f"tune {r['strategy']} member-updates/s"] = (r["member_updates_per_s"], True)
            elif what and "median_ms" in r:
                out[f"{what}{' pairs=%d' % r['pairs'] if 'pairs' in r else ''} median_ms"] = (r["median_ms"], False)
    return out


total = bad = 0
for tool in ("bench", "ens_time", "em_replay_time", "synth_time", "pbt_time"):
    runs = {}
    for f in glob.glob(os.path.join(d, f"{tool}_*.txt")):
        tag = os.path.basename(f)[len(tool) + 1:-4]
        runs[tag] = figures(tool, records(f))
    if len(runs) < 6:
        print(f"{tool}: {len(runs)} of 6 runs present, not summarised")
        continue
    print(f"{tool}: parent1 new1 parent2 new2 parent3 new3")
    for name, (_, hib) in runs["parent1"].items():
        par = [runs[f"parent{r}"][name][0] for r in (1, 2, 3)]
        new = [runs[f"new{r}"][name][0] for r in (1, 2, 3)]
        gap = max(abs(a - b) for a, b in zip(par, par[1:]))
        excess = (min(par) - min(new)) if hib else (max(new) - max(par))
        ok = excess <= gap
        total += 1
        bad += not ok
        print(f"  {name:42s} {'higher' if hib else 'lower '} is better  parent " + " ".join(f"{x:10.4f}" for x in par) +
              "  new " + " ".join(f"{x:10.4f}" for x in new) + f"  allowed {gap:9.4f} excess {excess:+9.4f}  {'ok' if ok else 'MISS'}")
print(f"figures missing the criterion: {bad} of {total}")
