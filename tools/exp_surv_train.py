"""One accumulation window of SURVIVAL bags (4 time bins, NLLSurvLoss(alpha = 0.4)), timed two ways in one process, alternating:
  native    FusedTrainer(loss="nll_surv").window_step: ONE call of mhimx_pure_window_run_surv / mhimx_ragged_window_run_surv per window
  autograd  the route a survival dataset had before those calls: CommonMIL.forward_func's autograd form with survival.NLLSurvLoss bag
            after bag (loss / n, backward()), then torch.optim.Adam.step(), zero_grad() and - full model - the EMA of the teacher
Legs (the sizes of tools/exp_pure_window.py and tools/exp_ragged_window.py, D = 1024, dropout 0.25):
  PA  teacher-free, 8 bags of 512 rows                         PC  teacher-free, 8 bags of 64 .. 4 000 rows (fixed seed)
  FA  full MHIM(ABMIL), 8 bags log-uniform in 500 .. 30 000 rows (fixed seed), the V2 recipe
Every leg: WARM windows of each route first, then REPS (>= 20) windows per route, one device-event pair around each window (the window
ends device-complete).  Prints one JSON line: per leg and route the median and min .. max in ms per window, and the route taken."""
import json, math, os, random, statistics, sys, types

sys.path.insert(0, os.environ.get("REPO") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mhim_mil_amd import synth
from mhim_mil_amd.engine import CommonMIL, FusedTrainer
from mhim_mil_amd.mhim import MHIM
from mhim_mil_amd.survival import NLLSurvLoss

D, K, ALPHA, MM = 1024, 4, 0.4, 0.9997
REPS = max(20, int(os.environ.get("REPS", 24)))
WARM = int(os.environ.get("WARM", 3))
LEGS = os.environ.get("LEGS", "PA,PC,FA").split(",")
dev = torch.device("cuda", 0)
V2 = dict(act="gelu", da_act="relu", mask_ratio_h=0.03, mask_ratio_hr=0.5, attn2score=True, merge_enable=True, merge_k=5, merge_mm=0.9999,
          merge_ratio=0.9, temp_t=0.1, dropout=0.25)


def pure_model():
    m = MHIM(input_dim=D, n_classes=K, baseline="attn", act="gelu", da_act="relu", merge_enable=False, dropout=0.25)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in synth.mhim_state(7, input_dim=D, n_classes=K, merge_enable=False).items()})
    return m.to(dev).train()


def full_models():
    base = synth.mhim_state(7, input_dim=D, n_classes=K, merge_k=5)
    out = []
    for sd in (base, synth.spread_teacher(base)):
        m = MHIM(input_dim=D, n_classes=K, baseline="attn", **V2)
        sd = dict(sd)
        sd["merge.global_q"] = sd["merge.global_q_mm"]
        m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()})
        m = m.to(dev).train()
        m.merge.dropout = 0.0
        out.append(m)
    return out


def autograd_window(kind, model, ema, opt, bags, labels, it):
    """engines/base_engine.py:395-441 for one window: forward_func, the criterion, loss / n, backward(); one optimiser step; the EMA"""
    args = types.SimpleNamespace(model=kind, baseline="attn", aux_alpha=0.5 if kind == "mhim" else 0.0)
    eng, crit, n = CommonMIL(args), NLLSurvLoss(alpha=ALPHA), len(bags)
    for x, lab in zip(bags, labels):
        logits, lab, aux, _, _, _, _ = eng.forward_func(args, model, ema, x, lab, crit, 1, it, 0, it, None)
        loss = (crit(logits=logits, Y=lab[0], c=lab[1]) + args.aux_alpha * aux) / n
        loss.backward()
    opt.step()
    opt.zero_grad(set_to_none=True)
    if ema is not None:
        with torch.no_grad():
            ps, pt = list(model.parameters()), list(ema.parameters())
            torch._foreach_mul_(pt, MM)
            torch._foreach_add_(pt, ps, alpha=1.0 - MM)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


g = torch.Generator(device=dev); g.manual_seed(5)
small = [random.Random(17 + j).randint(64, 4000) for j in range(8)]
rng = random.Random(11)
logu = [int(round(math.exp(rng.uniform(math.log(500), math.log(30000))))) for _ in range(8)]
x0 = torch.randn(max(logu), D, device=dev, generator=g).abs_()
sizes = {"PA": [512] * 8, "PC": small, "FA": logu}
labels = [[torch.tensor([j % K], device=dev), torch.tensor([float(j % 3 == 0)], device=dev)] for j in range(8)]
out = {"reps": REPS, "warm": WARM, "ms_per_window": {}, "exec": {}, "sizes": sizes}
for leg in LEGS:
    kind = "mhim" if leg.startswith("F") else "mhim_pure"
    bags = [x0[:n].unsqueeze(0) for n in sizes[leg]]
    if kind == "mhim":
        s, t = full_models()
        tr = FusedTrainer(s, t, aux_alpha=0.5, mm=MM, accumulation_steps=8, loss="nll_surv", surv_alpha=ALPHA)
        model, ema = full_models()
        for p in ema.parameters():
            p.requires_grad_(False)
    else:
        tr = FusedTrainer(pure_model(), None, model="mhim_pure", accumulation_steps=8, loss="nll_surv", surv_alpha=ALPHA)
        model, ema = pure_model(), None
    opt = torch.optim.Adam(model.parameters(), lr=2e-4, weight_decay=1e-5)
    pairs = [(l[0], l[1]) for l in labels]
    routes = {"native": lambda: tr.window_step(bags, pairs), "autograd": lambda it=[0]: autograd_window(kind, model, ema, opt, bags, labels, it[0])}
    for _ in range(WARM):
        for fn in routes.values():
            fn()
    torch.cuda.synchronize()
    out["exec"][leg] = str(tr.last.get("exec"))
    ms = {name: [] for name in routes}
    for _ in range(REPS):                                           # alternating: both routes see the same minutes of the machine
        for name, fn in routes.items():
            ms[name].append(timed(fn))
    out["ms_per_window"][leg] = {name: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}
                                 for name, v in ms.items()}
    del tr, model, ema, opt, routes
    torch.cuda.empty_cache()
print(json.dumps(out))
