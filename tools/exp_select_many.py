"""The production select of every bag of a ragged window in one call (mhimx_select_rows_many): what it saves, on windows of 8 and of 32
bags (D = 1024, the V2 recipe, seeded sizes: 8 bags log-uniform in 500 .. 16 000 rows, 32 bags uniform in 64 .. 2 000 rows).

    leg S8 / S32   the row lists alone, on device-resident scores: a Python loop of ops.select_rows (form "loop") against ONE
                   ops.select_rows_many (form "many"; only where the checkout has it), the forms alternated inside one process
    leg W8 / W32   FusedTrainer.window_step on the ragged route (mhimx_ragged_window_run), 4 rotating windows: the route is whatever the
                   checkout that is imported does (REPO=<checkout> selects it)

    python tools/exp_select_many.py                          one process: every leg, ROUNDS windows of at least WINDOW_S seconds each (each
                                                             ends in a device synchronise), one JSON line
    python tools/exp_select_many.py --against PARENT [--md profiles/select_many.md]
                                                             the protocol: PASSES times {this checkout, the parent checkout at PARENT} as
                                                             fresh processes one after the other (alternated), then the summary - median and
                                                             min .. max per leg, form and checkout; the parent's own min .. max over its passes
                                                             is the spread a difference has to exceed; --md APPENDS the
                                                             run (table + raw lines) to the file, which may be a document
    python tools/exp_select_many.py --summarize a.jsonl ...  the summary of collected lines
No time is claimed here: the figure of merit is the parent checkout's route on the same machine in the same call."""
import json, math, os, random, statistics, subprocess, sys, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def summarize(lines):
    res = {}
    for d in lines:
        for leg, forms in d["ms"].items():
            for form, v in forms.items():
                res.setdefault(leg, {}).setdefault(f"{d['route']}:{form}", []).extend(v)
    out = ["| leg | checkout : form | n | median ms | min .. max |", "|---|---|---|---|---|"]
    for leg, forms in sorted(res.items()):
        for name, v in sorted(forms.items()):
            out.append(f"| {leg} | {name} | {len(v)} | {statistics.median(v):.4f} | {min(v):.4f} .. {max(v):.4f} |")
    verdicts = []
    for leg, forms in sorted(res.items()):
        names = sorted(forms)
        for i, ra in enumerate(names):
            for rb in names[i + 1:]:
                a, b = forms[ra], forms[rb]
                apart = max(a) < min(b) or max(b) < min(a)
                verdicts.append(f"{leg}: {ra} / {rb}: ranges {'do NOT overlap' if apart else 'OVERLAP'}; median ratio "
                                f"{statistics.median(a) / statistics.median(b):.3f}")
    return out, verdicts


if len(sys.argv) > 1 and sys.argv[1] == "--summarize":
    rows = [json.loads(l) for p in sys.argv[2:] for l in open(p) if l.strip().startswith("{")]
    table, verdicts = summarize(rows)
    print("\n".join(table + [""] + verdicts))
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--against":
    parent = os.path.abspath(sys.argv[2])
    md = sys.argv[sys.argv.index("--md") + 1] if "--md" in sys.argv else ""
    passes = int(os.environ.get("PASSES", 3))
    rows = []
    for p in range(passes):
        for route, repo in (("new", HERE), ("parent", parent)):             # fresh processes, one at a time, alternated
            env = dict(os.environ, REPO=repo, ROUTE_NAME=route)
            r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"pass {p} of {route} ended with status {r.returncode}:\n{r.stderr[-2000:]}")
            line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
            print(line, flush=True)
            rows.append(json.loads(line))
    table, verdicts = summarize(rows)
    text = "\n".join(table + [""] + [f"- {v}" for v in verdicts])
    print(text, flush=True)
    if md:                                                                  # appended: the file may be a document that holds more than this run
        with open(md, "a") as f:
            f.write(f"\n## Run of {time.strftime('%Y-%m-%d %H:%M')}, PASSES={passes}\n\n" + text + "\n\n```json\n"
                    + "\n".join(json.dumps(r) for r in rows) + "\n```\n")
    sys.exit(0)

sys.path.insert(0, os.environ.get("REPO") or HERE)
import torch
from mhim_mil_amd import ops, synth
from mhim_mil_amd.mhim import MHIM
from mhim_mil_amd.engine import FusedTrainer

D = 1024
ROUNDS = int(os.environ.get("ROUNDS", 5))
WINDOW_S = float(os.environ.get("WINDOW_S", 0.5))
LEGS = os.environ.get("LEGS", "S8,S32,W8,W32").split(",")
dev = torch.device("cuda", 0)
CFG = dict(act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5, attn2score=True, merge_enable=True, merge_k=5, merge_mm=0.9999,
           merge_ratio=0.9, temp_t=0.1, dropout=0.25)
base = synth.mhim_state(7, input_dim=D, merge_k=5)


def model(sd):
    m = MHIM(input_dim=D, n_classes=2, baseline="attn", **CFG)
    sd = dict(sd)
    sd["merge.global_q"] = sd["merge.global_q_mm"]
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
    m = m.to(dev).train()
    m.merge.dropout = 0.0
    return m


def timed(fns, per_call=1):
    """ms per call of every function of fns in turn, over and over, for at least WINDOW_S seconds (device-complete)."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for f in fns:
            f()
        n += len(fns) * per_call
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= WINDOW_S:
            return dt / n * 1e3


g = torch.Generator(device=dev); g.manual_seed(5)
rnd = random.Random(3)
sizes = {8: [[int(round(math.exp(rnd.uniform(math.log(500), math.log(16000))))) for _ in range(8)] for _ in range(4)],
         32: [[rnd.randint(64, 2000) for _ in range(32)] for _ in range(4)]}
x0 = torch.randn(16000, D, device=dev, generator=g).abs_()
labels = [torch.tensor([j % 2], device=dev) for j in range(32)]
out = {"route": os.environ.get("ROUTE_NAME", "new"), "rounds": ROUNDS, "window_s": WINDOW_S, "ms": {}, "exec": {}, "sizes": sizes,
       "unit": {"S": "ms per window's row lists", "W": "ms per window_step"}}
mdl = model(base)
tick = torch.full((1,), 17, dtype=torch.int64, device=dev)
for leg in LEGS:
    n = int(leg[1:])
    if leg[0] == "S":
        tables = []
        for ns in sizes[n]:
            score = torch.rand(sum(ns), device=dev, generator=g)
            tab, r0, o0 = [], 0, 0
            for j, N in enumerate(ns):
                k, n_sel, len_keep, Lk, R = mdl.v2_counts(N)
                tab.append((r0, N, k, n_sel, R, o0, 1000 + j))
                r0, o0 = r0 + N, o0 + len_keep
            tables.append((score, tab, torch.empty(o0, dtype=torch.int64, device=dev)))

        def loop(score, tab, rows):
            for r0, N, k, n_sel, R, o0, seed in tab:
                ops.select_rows(score[r0:r0 + N], k, n_sel, R, seed, tick=tick, merge_first=True, out=rows[o0:o0 + N - n_sel])

        forms = {"loop": [lambda t=t: loop(*t) for t in tables]}
        if hasattr(ops, "select_rows_many"):
            forms["many"] = [lambda t=t: ops.select_rows_many(t[0], t[1], tick=tick, merge_first=True, out=t[2]) for t in tables]
            for score, tab, rows in tables:                                 # the two forms write the same lists
                loop(score, tab, rows)
                want = rows.clone()
                rows.fill_(-1)
                ops.select_rows_many(score, tab, tick=tick, merge_first=True, out=rows)
                assert torch.equal(rows, want), "select_rows_many differs from the select_rows loop"
    else:
        tr = FusedTrainer(model(base), model(synth.spread_teacher(base)), aux_alpha=0.5, mm=0.9997, accumulation_steps=n)
        wins = [[x0[:N] for N in ns] for ns in sizes[n]]
        forms = {"window_step": [lambda w=w: tr.window_step(w, labels[:n]) for w in wins]}
    out["ms"][leg] = {}
    for name, fns in forms.items():                                         # warm every shape
        for f in fns:
            f()
        torch.cuda.synchronize()
        out["ms"][leg][name] = []
    if leg[0] == "W":
        out["exec"][leg] = str(tr.last.get("exec"))
        assert out["exec"][leg] == "mhimx_ragged_window_run", out["exec"][leg]
    for _ in range(ROUNDS):                                                 # the forms of a leg alternate
        for name, fns in forms.items():
            out["ms"][leg][name].append(round(timed(fns), 5))
    if leg[0] == "W":
        del tr
    del forms
    torch.cuda.empty_cache()
print(json.dumps(out))
