"""Train-step API for the MHIM path.

``CommonMIL`` mirrors the hook object the reference trainer calls (engines/common_mil.py:1-68): same
method names, keyword arguments and return tuples, so ``BaseTrainer.train/validate`` can drive the HIP
model unchanged.

``FusedTrainer`` is the MI355X-native step the benchmark times: teacher forward -> select -> student
forward -> head (CE + distillation) -> hand-derived backward -> [RCCL all-reduce of ONE flat gradient
buffer] -> fused Adam + EMA-teacher kernel.  It bypasses autograd and the per-parameter Python loops of
base_engine.py:155-167 (one flat fp32 buffer each for student, teacher, gradient, Adam m and v), which is
what makes a tens-of-microseconds bag step reachable at all.
"""
from __future__ import annotations

from typing import Optional

import collections
import contextlib
import dataclasses
import os

import torch

from . import mhim as mh
from . import ops
from .mhim import MHIM, BagPlan


class CommonMIL:
    """Hook object of the reference trainer (engines/common_mil.py)."""

    def __init__(self, args=None, fused=None, graph_cache=0) -> None:
        self.training = True
        self.fused = fused                 # optional optim.FusedAdamEMA: forward_func may run the native forward + backward (its docstring)
        # graph_cache = K > 0 (with fused=): the native forward + backward of the K most recent bag SHAPES as captured hipGraphs - the second
        # bag of a shape is captured (into buffers of its own: the bag is copied in, one launch), every later one replays; other shapes
        # run eagerly as before.  MHIM(ABMIL), one process, accumulation_steps == 1 (FusedTrainer.shape_cached).
        self.graph_cache = int(graph_cache)

    def _native_step(self, tr, bag, label, n_iter, extra):
        """The native forward + backward of one bag: a replay of the shape's captured graph when there is one (graph_cache), else eager."""
        if self.graph_cache > 0 and not extra:
            out = tr.shape_cached("forward_backward", bag, label, i=n_iter, cache=self.graph_cache)
            if out is not None:
                return out
        logits, losses = tr.forward_backward(bag, label, i=n_iter, **extra)
        return logits, losses, tr.last["patch_num"], tr.last["keep_num"]

    def init_func_train(self, args, **kwargs):
        self.training = True

    def init_func_val(self, args, **kwargs):
        self.training = False

    def after_get_data_func(self, args, **kwargs):
        pass

    def after_backward_func(self, args, **kwargs):
        pass

    def final_train_func(self, args, **kwargs):
        pass

    def forward_func(self, args, model, model_ema, bag, label, criterion, batch_size, i, epoch, n_iter, pos, **kwargs):
        """-> (logits, label, aux_loss, patch_num, keep_num, pad_ratio, kn_std)   (common_mil.py:14-48)"""
        dsmil = getattr(args, "baseline", "attn") == "dsmil"
        fz = self.fused
        if (fz is not None and model is fz.model and model_ema is fz.model_ema and model.training and not dsmil
                and args.model == fz.trainer.model_kind and type(criterion) is torch.nn.CrossEntropyLoss and criterion.weight is None
                and criterion.label_smoothing == 0.0 and criterion.reduction == "mean" and batch_size == 1):
            # the loop's loss is main_alpha * CE + aux_alpha * aux (/ accumulation_steps), base_engine.py:99-102: the native step computes
            # exactly that and its gradient (no autograd graph); the loop gets LEAVES - its criterion / backward touch no parameter
            tr = fz.trainer
            tr.main_alpha, tr.aux_alpha = float(getattr(args, "main_alpha", 1.0)), float(args.aux_alpha)
            extra = {k: kwargs[k] for k in ("perm", "ids_shuffle") if k in kwargs}
            logits, losses, patch_num, keep_num = self._native_step(tr, bag, label.view(-1)[:1], n_iter, extra)
            lg = logits.detach().view(batch_size, -1).clone().requires_grad_(True)     # (clone: a replay rewrites the graph's buffers)
            aux = losses[2].detach().clone().requires_grad_(True)
            return lg, label, aux, patch_num, keep_num, 0., 0.
        if (fz is not None and model is fz.model and model_ema is fz.model_ema and model.training and not dsmil
                and args.model == fz.trainer.model_kind and fz.trainer.loss == "nll_surv" and batch_size == 1
                and isinstance(label, (list, tuple)) and len(label) == 2):
            from .survival import NLLSurvLoss
            if type(criterion) is NLLSurvLoss:
                # the survival loop's loss is main_alpha * NLLSurvLoss(alpha)(logits, Y, c) + aux_alpha * aux (engines/base_engine.py:395-441):
                # the native step computes exactly that and its gradient; the loop gets LEAVES, as in the cross-entropy branch above
                tr = fz.trainer
                tr.main_alpha, tr.aux_alpha, tr.surv_alpha = float(getattr(args, "main_alpha", 1.0)), float(args.aux_alpha), float(criterion.alpha)
                dev = tr.flat.student.device
                Y = label[0].reshape(-1)[:1].to(device=dev, dtype=torch.int64).contiguous()
                c = label[1].reshape(-1)[:1].to(device=dev, dtype=torch.float32).contiguous()
                extra = {k: kwargs[k] for k in ("perm", "ids_shuffle") if k in kwargs}
                logits, losses = tr.forward_backward(bag, (Y, c), i=n_iter, **extra)
                lg = logits.detach().view(batch_size, -1).clone().requires_grad_(True)
                aux = losses[2].detach().clone().requires_grad_(True)
                return lg, label, aux, tr.last["patch_num"], tr.last["keep_num"], 0., 0.
        if args.model == "mhim":
            teacher_feat, score = (None, None)
            if model_ema is not None:
                teacher_feat, score = model_ema.forward_teacher(bag)
            if args.aux_alpha == 0.:
                teacher_feat = None                                        # common_mil.py:24
            if dsmil and teacher_feat is not None:
                teacher_feat = teacher_feat[0]                              # common_mil.py:27: cls_tea[0] = B [C,E]
            # the reference trainer calls forward_func with loader=, device=, others=, idx=, feat= ... (base_engine.py:77-93) and its
            # CommonMIL hands none of them to the model (common_mil.py:30); only the parity tests' injected draws go through
            extra = {k: kwargs[k] for k in ("perm", "ids_shuffle", "drop_mask") if k in kwargs}
            logits, aux_loss, patch_num, keep_num = model(bag, score, teacher_feat, i=n_iter, **extra)
            if dsmil:                                                       # common_mil.py:28
                logits = 0.5 * logits[0].view(batch_size, -1) + 0.5 * logits[1].view(batch_size, -1)
        elif args.model == "mhim_pure":
            logits, aux_loss, patch_num, keep_num = model.pure(bag)
            if dsmil:                                                       # common_mil.py:34-35
                logits = 0.5 * logits[0].view(batch_size, -1) + 0.5 * logits[1].view(batch_size, -1)
        else:
            raise NotImplementedError(f"model {args.model!r} is outside the MHIM hot path")
        return logits, label, aux_loss, patch_num, keep_num, 0., 0.

    def validate_func(self, args, model, bag, label, criterion, batch_size, i, pos, epoch=None, **kwargs):
        """-> (logits, label)   (common_mil.py:56-68)"""
        if args.model not in ("mhim", "mhim_pure"):
            raise NotImplementedError(f"model {args.model!r} is outside the MHIM hot path")
        logits = model.forward_test(bag)
        if getattr(args, "baseline", "attn") == "dsmil":                    # common_mil.py:59-60,66-67
            logits = logits[0]
            logits = 0.5 * logits[0] + 0.5 * logits[1]
        return logits, label


    def validate_many(self, args, model, bags, labels, criterion=None):
        """validate_func for a LIST of bags -> (logits [n, C], per-bag cross entropy [n] | None).  The MHIM models go through
        MHIM.infer_many (one C call per chunk of bags where the model qualifies - ABMIL and DSMIL -, the forward_test loop where it does
        not; for DSMIL the logits are validate_func's 0.5 / 0.5 mix either way); the loss comes back only for a plain CrossEntropyLoss -
        any other criterion is the caller's to apply to the logits."""
        if args.model not in ("mhim", "mhim_pure"):
            raise NotImplementedError(f"model {args.model!r} is outside the MHIM hot path")
        if not hasattr(model, "infer_many"):
            rows = [self.validate_func(args, model=model, bag=b, label=labels[j:j + 1], criterion=criterion, batch_size=1, i=j, pos=None)[0]
                    for j, b in enumerate(bags)]
            return torch.cat([r.reshape(1, -1) for r in rows]), None
        plain = (type(criterion) is torch.nn.CrossEntropyLoss and criterion.weight is None and criterion.label_smoothing == 0.0
                 and criterion.reduction == "mean" and criterion.ignore_index < 0)
        if plain:
            return model.infer_many(bags, labels=labels)
        return model.infer_many(bags), None


def cosine_scheduler(base_value, final_value, epochs, niter_per_ep, warmup_epochs=0, start_warmup_value=0):
    """The reference's per-iteration cosine schedule (utils.py:199-210): used for `mm_sche` (EMA momentum mm -> 1,
    modules/__init__.py:177-181) and `mrh_sche` (HAM ratio mask_ratio_h -> 0, modules/__init__.py:72-75)."""
    import numpy as np
    warmup_iters = warmup_epochs * niter_per_ep
    warm = np.linspace(start_warmup_value, base_value, warmup_iters) if warmup_epochs > 0 else np.array([])
    iters = np.arange(epochs * niter_per_ep - warmup_iters)
    sched = final_value + 0.5 * (base_value - final_value) * (1 + np.cos(np.pi * iters / len(iters)))
    sched = np.concatenate((warm, sched))
    assert len(sched) == epochs * niter_per_ep
    return sched


class FlatState:
    """Flat fp32 buffers behind a student/teacher pair.

    Layout: [trainable parameters in named_parameters() order | non-trainable parameters (merge.global_q_mm)].
    Every nn.Parameter of both models becomes a view into its flat buffer, so state_dict()/load_state_dict()
    keep working and the fused optimiser touches each byte once.
    """

    def __init__(self, student: MHIM, teacher: Optional[MHIM], step_merges=True):
        named = list(student.named_parameters())          # de-duplicated (global_q alias appears once)
        # parameters the forward never touches get no gradient; torch.optim.Adam skips those (no update, no weight decay),
        # so they sit in the non-trainable tail here (DSMIL never uses MHIM.predictor: mhim.py:264-265)
        unused = set(getattr(student, "unused_parameter_names", lambda: ())())
        if not step_merges:                               # 'mhim_pure' never calls Merge: its parameters get no gradient either
            unused |= {n for n, _ in named if n.startswith("merge.")}
        self.train_names = [n for n, p in named if p.requires_grad and n not in unused]
        # the projection's weight and bias lead the buffer: their gradient is the last to become final in a backward, so a data-
        # parallel step all-reduces [the rest] first, overlapped with the projection's weight-gradient GEMM (FusedTrainer._mid_hook)
        head = [n for n in ("feature.0.weight", "feature.0.bias") if n in self.train_names]
        self.train_names = head + [n for n in self.train_names if n not in head]
        self.fixed_names = [n for n, p in named if not p.requires_grad or n in unused]
        self.names = self.train_names + self.fixed_names
        dev = named[0][1].device
        sizes = {n: p.numel() for n, p in named}
        self.offsets, off = {}, 0
        for n in self.names:
            self.offsets[n] = off
            off += (sizes[n] + 3) // 4 * 4                  # keep every tensor 16-byte aligned
            if n == self.train_names[-1]:
                self.n_train = off
        self.n_all = (off + 63) // 64 * 64         # (a multiple of every world size up to 64: the mesh form of the gradient exchange -
        self.student = self._adopt(student, dev)   #  reduce-scatter + all-gather on count / world slices - takes the whole buffer)
        # --tea_type same (modules/__init__.py:211-212: the teacher IS the student; base_engine.py:157-158: no EMA): one buffer, adopted once
        self.same_teacher = teacher is not None and teacher is student
        self.teacher = self.student if self.same_teacher else (self._adopt(teacher, dev) if teacher is not None else None)
        self.grad = torch.zeros(self.n_all, device=dev)
        self.m = torch.zeros(self.n_train, device=dev)
        self.v = torch.zeros(self.n_train, device=dev)
        self.grad_views = {}
        pd = dict(student.named_parameters())
        for n in self.train_names:
            self.grad_views[n] = self.grad[self.offsets[n]:self.offsets[n] + sizes[n]].view_as(pd[n])
        self.step = 0

    def _adopt(self, model, dev):
        flat = torch.zeros(self.n_all, device=dev)
        pd = dict(model.named_parameters())
        for n in self.names:
            p = pd[n]
            view = flat[self.offsets[n]:self.offsets[n] + p.numel()].view_as(p)
            view.copy_(p.data)
            p.data = view
        return flat


class QueryChain:
    """How Merge's in-forward EMA of the global queries (merge.py:142-143) composes over the ranks of a data-parallel update.

    A single process with accumulation_steps = W runs the EMA bag after bag: q <- mm q + (1 - mm) z_r, r = 0 .. W-1.  W ranks each see
    the step's first queries q0 (nothing orders them), so the same chain is applied to the tokens z_r their forwards produced:
        q <- mm^W q0 + (1 - mm) sum_r mm^(W-1-r) z_r
    - rank r puts w_r z_r, w_r = (1 - mm) mm^(W-1-r), into its slice of the flat buffer's tail, the ONE SUM all-reduce adds them, and
    every rank finishes with mm^W q0 + the sum.  The same contract as an accumulation window (FusedTrainer.window_step, oracle
    ``train_window(q_ema="window")``): it differs from the bag-after-bag order only through d z_r / d q (second order in 1 - mm), where
    averaging the ranks' one-step results would slow the EMA down W-fold (first order)."""

    def __init__(self, offset, numel, mm, world, rank):
        self.off, self.n = int(offset), int(numel)
        self.w = (1.0 - mm) * mm ** (world - 1 - rank)
        self.decay = mm ** world
        self.tokens = None                       # [k, E] tokens of this rank's forward (set by the step)


def sync_flat_gradient(grad: torch.Tensor, student: torch.Tensor, n_train: int, world: int, group=None, comm=None, chain: QueryChain = None) -> float:
    """The ONE collective of a data-parallel update (RCCL on GPUs; any backend works, gloo in the CPU tests).

    Everything that must agree across ranks rides in the same flat buffer: the gradient (first n_train floats) and,
    in the tail, the non-trainable parameters that each rank mutated in its own forward (merge.global_q_mm's EMA,
    merge.py:142-143).  After the SUM all-reduce the tail is averaged back into ``student``; the
    returned scale (1/world) is applied to the gradient inside the fused Adam kernel.  No data-path collective exists:
    bags are independent units.  ``comm``: a ``comm.NativeComm`` (the C-ABI's own RCCL handle, ``mhimx_comm_allreduce``) instead of
    torch.distributed - the same collective for hosts that do not run torch.distributed.
    """
    if world <= 1:
        return 1.0
    fill_tail(grad, student, n_train, chain)
    if comm is not None:
        comm.allreduce(grad)
    else:
        torch.distributed.all_reduce(grad, group=group)
    scale = 1.0 / world
    finish_tail(grad, student, n_train, scale, chain)
    return scale


def fill_tail(grad, student, n_train, chain=None):
    """Before the SUM: the tail of the flat buffer carries the non-trainable parameters (averaged back afterwards); with a QueryChain
    the global queries' slice carries this rank's weighted tokens instead."""
    grad[n_train:].copy_(student[n_train:])
    if chain is not None and chain.tokens is not None:
        torch.mul(chain.tokens.reshape(-1), chain.w, out=grad[chain.off:chain.off + chain.n])


def finish_tail(grad, student, n_train, scale, chain=None):
    if chain is not None and chain.tokens is not None:
        q0 = student[chain.off:chain.off + chain.n].clone()
        student[n_train:].copy_(grad[n_train:] * scale)
        torch.add(grad[chain.off:chain.off + chain.n], q0, alpha=chain.decay, out=student[chain.off:chain.off + chain.n])
        chain.tokens = None
    else:
        student[n_train:].copy_(grad[n_train:] * scale)
    grad[n_train:].zero_()


# Accumulation windows: both GEMMs of the window's bags as ONE launch each (mhimx_bag_project_multi / mhimx_bag_wgrad_multi).  MEASURED
# (round 3, 8 bags of the c2 shape, same box): the projection 8 x 61.2 -> 470 us, the weight gradient 8 x (44 + 3 of slab sum) -> 219 us -
# (tools/exp_wgrad_multi.py) and the window not at all (1.52 ms on 4 streams, 2.55 ms on one, with or without): the Merge backward's tail that rode in each bag's
# weight-gradient launch becomes a launch of its own (8 x 17.8 us), and the window on 4 streams is bound by how the graph's branches
# overlap (average concurrency 1.7, profiles/r03_window_timeline.md), not by kernel time.  Opt-in until the tail rides elsewhere.
_STEP_IMAGES = os.environ.get("MHIMX_STEP_IMAGES", "1") != "0"       # TransMIL: the step's weight images in the preparation launch
_WINDOW_BATCHED = os.environ.get("MHIMX_WINDOW_BATCHED", "1") != "0"      # (round 6) mhimx_window_run for windows of same-shaped bags
_WINDOW_WGRAD = os.environ.get("MHIMX_WINDOW_WGRAD", "0") != "0"
_WINDOW_PROJECT = os.environ.get("MHIMX_WINDOW_PROJECT", "0") != "0"


class _SplitStep:
    """A captured data-parallel step: graph(forward + backward + tail fill) -> eager all-reduce of the flat buffer -> graph(tail
    average + Adam + EMA)."""

    def __init__(self, trainer, g_fb, g_up):
        self.tr, self.g_fb, self.g_up = trainer, g_fb, g_up

    def replay(self):
        tr = self.tr
        self.g_fb.replay()                                     # ... + the buffer's tail filled
        tr._all_reduce(tr.flat.grad)
        self.g_up.replay()                                     # the tail averaged back + Adam + EMA
        ops.step_images(None)                                  # (nothing on the host installed any; a replay must not leave any either)


# ------------------------------------------------------------------------------------------------- the four ragged native train calls
@dataclasses.dataclass(frozen=True)
class _WindowFamily:
    """What differs between the four native calls that make one update over 1 .. 32 bags of different row counts; FusedTrainer._run_family,
    _family_ok, _window_rows_ok and _native_form hold what they share.  The trainer's methods and attributes are named, not bound:
    tests replace ``ok`` and ``run`` on an instance."""
    model_kind: str                 # the trainer's model and
    baseline: str                   # the student's baseline the call serves
    ok: str                         # the trainer's check,
    run: str                        # its call,
    shapes: str                     # its static mirror of the C checks,
    row_cap: str                    # its cap on the rows of a call's row space,
    cfg: str                        # its cfg builder, whose {"key", "cfg", ...} also caches the workspace at
    ws_key: str
    layout_of: object               # ops: (cfg, table, n) -> the layout; host arithmetic only
    call: object                    # ops: (cfg, table, n, host_step, ws, update, x_dtype=[, surv=])
    exec: object                    # last["exec"]
    exec_surv: object               # last["exec"] of the call's survival form (None: it has none)
    full: bool                      # the full model: RaggedWindowBag rows (counts, _step_seeds), ok / run take ``i``, last is the last bag's
    #                                 views + "table"; else PureWindowBag rows (one dropout seed) made by
    table: object                   # ops: (xs, labels, seeds) -> the rows, and last is _last_pure of the last bag
    views: object                   # (trainer, ws, layout, xs, table) -> the bags' dictionaries of workspace views
    max_bags: int                   # include/mhimx.h's bounds of the call
    max_rows: int
    accum_caps_bags: bool           # see _DSMIL
    feature_bf16x3: bool            # every bag's feature precision must be "bf16x3"
    trainer_ok: object              # (trainer, n bags) -> the family's own trainer and model conditions
    bags_ok: object                 # (trainer, xs, i, device) -> its parameter / per-bag conditions, behind the labels' (None: none)


def _plain_views(tr, ws, lay, xs, table, dsmil=False):
    """The bags of a teacher-free call: logits, losses, feature rows and their dropout / activation image; DSMIL: its two heads, B, crit."""
    s, view, n = tr.s, ops.ws_view, len(xs)
    E, Cc = s.mlp_dim, s.n_classes
    lg, ls = view(ws, lay.logits, n * Cc).view(n, Cc), view(ws, lay.losses, n * 3).view(n, 3)
    if dsmil:
        lb, li = view(ws, lay.logits_bag, n * Cc).view(n, Cc), view(ws, lay.logits_ins, n * Cc).view(n, Cc)
        B, crit = view(ws, lay.B, n * Cc * E).view(n, Cc, E), view(ws, lay.crit, n * Cc, torch.int64).view(n, Cc)
    H = view(ws, lay.H, lay.rows * E).view(lay.rows, E)
    dact = view(ws, lay.dact, lay.rows * E, torch.float16).view(lay.rows, E)
    per = []
    for j, x in enumerate(xs):
        r0, N = int(lay.row0[j]), x.shape[0]
        heads = {"logits_bag": lb[j], "logits_ins": li[j], "B": B[j], "crit": crit[j]} if dsmil else {}
        per.append({"logits": lg[j], "losses": ls[j], **heads, "patch_num": N, "keep_num": N, "row0": r0, "H_student": H[r0:r0 + N],
                    "dact": dact[r0:r0 + N]})
    return per


def _dsmil_mhim_views(tr, ws, lay, xs, table):
    s, view, n = tr.s, ops.ws_view, len(xs)
    E, Cc, km = s.mlp_dim, s.n_classes, s.merge.k
    lg, ls = view(ws, lay.logits, n * Cc).view(n, Cc), view(ws, lay.losses, n * 3).view(n, 3)
    lb, li = view(ws, lay.logits_bag, n * Cc).view(n, Cc), view(ws, lay.logits_ins, n * Cc).view(n, Cc)
    B, Bt = view(ws, lay.B, n * Cc * E).view(n, Cc, E), view(ws, lay.B_teacher, n * Cc * E).view(n, Cc, E)
    crit = view(ws, lay.crit, n * Cc, torch.int64).view(n, Cc)
    Ht, Hs = view(ws, lay.H_teacher, lay.rows * E).view(lay.rows, E), view(ws, lay.H_student, lay.rows * E).view(lay.rows, E)
    dact = view(ws, lay.dact, lay.rows * E, torch.float16).view(lay.rows, E)
    score, rows_all = view(ws, lay.score, lay.rows), view(ws, lay.rows_all, lay.rows, torch.int64)
    T = view(ws, lay.tokens, lay.tok_rows * E).view(lay.tok_rows, E)
    per = []
    for j, x in enumerate(xs):
        r0, t0, N, cnt = int(lay.row0[j]), int(lay.tok0[j]), x.shape[0], table[j].cnt
        per.append({"logits": lg[j], "losses": ls[j], "logits_bag": lb[j], "logits_ins": li[j], "B": B[j], "B_teacher": Bt[j],
                    "score": score[r0:r0 + N], "rows": rows_all[r0:r0 + cnt.len_keep], "Lk": int(cnt.Lk), "R": int(cnt.R), "crit": crit[j],
                    "H_student": Hs[r0:r0 + N], "H_teacher": Ht[r0:r0 + N], "dact": dact[r0:r0 + N],
                    "tokens": T[t0 + cnt.Lk:t0 + cnt.Lk + km], "token_rows": T[t0:t0 + cnt.Lk + km], "row0": r0, "tok0": t0,
                    "patch_num": N, "keep_num": int(cnt.Lk) + km})
    return per


def _ragged_views(tr, ws, lay, xs, table):
    s, view, n = tr.s, ops.ws_view, len(xs)
    E, Cc = s.mlp_dim, s.n_classes
    lg, ls = view(ws, lay.logits, n * 16).view(n, 16), view(ws, lay.losses, n * 4).view(n, 4)
    dact = view(ws, lay.dact, lay.rows * E, torch.float16).view(lay.rows, E)
    zt, zs = view(ws, lay.z_teacher, n * E).view(n, E), view(ws, lay.z_student, n * E).view(n, E)
    per = []
    for j, x in enumerate(xs):
        r0, N = int(lay.row0[j]), x.shape[0]
        per.append(dict(tr._last_full(ws, lay, N, table[j].cnt, lg[j, :Cc], ls[j, :3], r0=r0), dact=dact[r0:r0 + N], z_teacher=zt[j],
                        z_student=zs[j], row0=r0))
    return per


def _dsmil_mhim_trainer_ok(tr, n):
    s, t = tr.s, tr.t
    return (t is not None and t.baseline == "dsmil" and tr._chain is None                  # check_dm refuses a q_out
            and 1 <= n <= tr.accum and s.training and s.merge_enable and not t.merge_test and s.mrh_sche is None and t._op_prec != "f32"
            and s.act == t.act and s.n_classes == t.n_classes)


def _ragged_trainer_ok(tr, n):
    s = tr.s
    # (a cross-entropy bag of accumulation_steps == 1 keeps mhimx_step_run; loss="nll_surv": there is no survival form of that call, a
    # single bag is a window of one)
    return ((tr.accum > 1 or tr.loss == "nll_surv") and 1 <= n <= tr.accum
            and tr._chain is None and not tr.step_dag and not tr.time_project                     # check_rw: q_out, side_stream, time_project
            and s.mrh_sche is None and s.merge_enable and s.merge.k <= 6)


def _dsmil_mhim_bags_ok(tr, xs, i, dev):
    s, mg = tr.s, tr.s.merge
    if not set(tr._DSMIL_PARAMS + tr._DSMIL_MERGE_PARAMS) <= set(tr.flat.train_names):
        return False
    mps = (mg.norm.weight.data, mg.norm.bias.data, mg.attn.to_kv.weight.data, mg.attn.to_q.weight.data, mg.attn.to_out[0].weight.data,
           mg.attn.to_out[0].bias.data, mg.global_q_mm.data)
    if (tuple(mps[2].shape) != (1024, 512) or tuple(mps[3].shape) != (512, 512) or tuple(mps[4].shape) != (512, 512)
            or mps[6].numel() != mg.k * 512 or any(not p.is_contiguous() or p.dtype != torch.float32 or p.device != dev for p in mps)
            or any(mps[j].data_ptr() % 16 for j in (0, 1, 2, 3, 4, 6))):
        return False
    # (w1_shape: the teacher is a model of its own - only the student's D and E reach dsmil_mhim_window_shapes_ok)
    return all(tr._dsmil_params_ok(m, dev, w1_shape=True) for m in (s, tr.t))


# FusedTrainer._window_route's answer: the route's name, the family of a native call (else None), the bags as the route reads them, the
# labels and the censorship flags (a survival call's) it takes
_Route = collections.namedtuple("_Route", "name fam xs labels surv")
# FusedTrainer._step_route's answer, its single-bag twin: "exec", "nat", "py", or a family's run with the family, its labels and flags
_StepRoute = collections.namedtuple("_StepRoute", "name fam labels surv")
# FusedTrainer.shape_cached's cache entry: the graph, its static bag / label / output buffers, self.last and the optimiser's scalars it baked in
_ShapeGraph = collections.namedtuple("_ShapeGraph", "graph x label logits losses patch_num keep_num last scal")

_L = mh.L
_PURE = _WindowFamily(
    "mhim_pure", "attn", ok="_pure_window_ok", run="_exec_pure_window", shapes="pure_window_shapes_ok", row_cap="pure_window_row_cap",
    cfg="_exec_cfg", ws_key="ws_pw", layout_of=ops.pure_window_layout, call=ops.pure_window_run, exec=True, exec_surv="mhimx_pure_window_run_surv",
    full=False, table=ops.pure_window_bags, views=_plain_views,
    max_bags=_L.PURE_WINDOW_MAX, max_rows=_L.PURE_WINDOW_MAX_ROWS, accum_caps_bags=False,       # check_pw (window_step bounds len(bags))
    feature_bf16x3=True,                                                                        # the call projects in the 3-term bf16 form only
    trainer_ok=lambda tr, n: tr.s.training and not tr.s.online_encoder.gated, bags_ok=None)
_DSMIL = _WindowFamily(
    "mhim_pure", "dsmil", ok="_dsmil_window_ok", run="_exec_dsmil_window", shapes="dsmil_window_shapes_ok", row_cap="dsmil_window_row_cap",
    cfg="_dsmil_cfg", ws_key="ws", layout_of=ops.dsmil_window_layout, call=ops.dsmil_window_run, exec="mhimx_dsmil_window_run", exec_surv=None,
    full=False, table=ops.dsmil_window_bags, views=lambda *a: _plain_views(*a, dsmil=True),
    max_bags=_L.DSMIL_WINDOW_MAX, max_rows=_L.DSMIL_WINDOW_MAX_ROWS,                            # check_dw
    accum_caps_bags=True,               # max_bags is min(accumulation_steps, max_bags), ONE bag at accumulation_steps == 1 (the others
    #                                     bound len(bags) by accumulation_steps in trainer_ok, or leave that to window_step)
    feature_bf16x3=True, trainer_ok=lambda tr, n: tr.s.training,
    # (every DSMIL tensor has a gradient view; what else the model carries - the unused predictor - has no gradient on any route)
    bags_ok=lambda tr, xs, i, dev: set(tr._DSMIL_PARAMS) <= set(tr.flat.train_names) and tr._dsmil_params_ok(tr.s, dev))
_DSMIL_MHIM = _WindowFamily(
    "mhim", "dsmil", ok="_dsmil_mhim_window_ok", run="_exec_dsmil_mhim_window", shapes="dsmil_mhim_window_shapes_ok",
    row_cap="dsmil_mhim_window_row_cap", cfg="_dsmil_mhim_cfg", ws_key="ws",
    layout_of=lambda cfg, table, n: ops.dsmil_mhim_window(cfg, table, n, layout_only=True), call=ops.dsmil_mhim_window,
    exec="mhimx_dsmil_mhim_window_run", exec_surv=None, full=True, table=None, views=_dsmil_mhim_views,
    max_bags=_L.DSMIL_MHIM_WINDOW_MAX, max_rows=_L.DSMIL_MHIM_WINDOW_MAX_ROWS, accum_caps_bags=False,     # check_dm
    feature_bf16x3=True, trainer_ok=_dsmil_mhim_trainer_ok, bags_ok=_dsmil_mhim_bags_ok)
_RAGGED = _WindowFamily(
    "mhim", "attn", ok="_ragged_window_ok", run="_exec_ragged_window", shapes="ragged_window_shapes_ok", row_cap="ragged_window_row_cap",
    cfg="_exec_cfg", ws_key="ws_rw", layout_of=lambda cfg, table, n: ops.ragged_window(cfg, table, n, layout_only=True), call=ops.ragged_window,
    exec="mhimx_ragged_window_run", exec_surv="mhimx_ragged_window_run_surv", full=True, table=None, views=_ragged_views,
    max_bags=_L.RAGGED_WINDOW_MAX, max_rows=_L.RAGGED_WINDOW_MAX_ROWS, accum_caps_bags=False,   # check_rw
    feature_bf16x3=False,                                                                       # check_cfg has no such rule: _exec_ok decides
    trainer_ok=_ragged_trainer_ok,
    bags_ok=lambda tr, xs, i, dev: all(tr._exec_ok(x, i, window=True) for x in xs))             # check_rw: check_cfg per bag


class FusedTrainer:
    """One-call MHIM(ABMIL) train step on flat buffers (the benchmarked path)."""

    def __init__(self, student: MHIM, teacher: Optional[MHIM], lr=2e-4, weight_decay=1e-5, betas=(0.9, 0.999), eps=1e-8,
                 mm=0.9997, main_alpha=1.0, aux_alpha=0.5, accumulation_steps=1, process_group=None, model="mhim", mm_sche=None,
                 clip_grad=None, lr_sche=None, loss="ce", surv_alpha=0.0, surv_eps=1e-7):
        if model not in ("mhim", "mhim_pure"):
            raise mh.L.MhimxError(f"FusedTrainer: model={model!r} (the path knows 'mhim' and 'mhim_pure')")
        if loss not in ("ce", "nll_surv"):
            raise mh.L.MhimxError(f"FusedTrainer: loss={loss!r} (the path knows 'ce' and 'nll_surv')")
        if loss == "nll_surv":
            # survival training (engines/base_engine.py:395-441, criterion train_utils.py:8-37): the ABMIL student with the plain scorer, one
            # process - the models mhimx_pure_window_run_surv / mhimx_ragged_window_run_surv serve.  Everything else keeps training through
            # CommonMIL.forward_func's autograd form
            if student.baseline != "attn" or getattr(student.online_encoder, "gated", False):
                raise mh.L.MhimxError(f"FusedTrainer(loss='nll_surv'): the ABMIL student with the plain scorer only (baseline="
                                      f"{student.baseline!r}, gated={getattr(student.online_encoder, 'gated', False)}); other models train "
                                      f"through CommonMIL.forward_func's autograd form")
            if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                             and torch.distributed.get_world_size() > 1):
                raise mh.L.MhimxError("FusedTrainer(loss='nll_surv'): one process (world > 1 trains through CommonMIL.forward_func's autograd form)")
            if not (0.0 <= float(surv_alpha) <= 1.0 and 0.0 < float(surv_eps) < 1.0):
                raise mh.L.MhimxError(f"FusedTrainer(loss='nll_surv'): surv_alpha={surv_alpha} must be in [0, 1], surv_eps={surv_eps} in (0, 1)")
        # loss="nll_surv": a label is a pair (Y, c) - the time bin (int64 [1]) and the censorship flag (fp32 [1]) as device tensors
        self.loss, self.surv_alpha, self.surv_eps = loss, float(surv_alpha), float(surv_eps)
        if model == "mhim" and teacher is None:
            raise mh.L.MhimxError("FusedTrainer(model='mhim') needs the EMA teacher (modules/__init__.py:176-214 builds it)")
        if model == "mhim" and not student.merge_enable:
            raise mh.L.MhimxError("FusedTrainer(model='mhim') needs merge_enable=True: the reference's MHIM.forward rejects the Identity "
                                  "merge (mhim.py:82,351)")
        self.s, self.t = student, teacher
        self.flat = FlatState(student, teacher, step_merges=(model == "mhim"))
        self.lr, self.wd, self.betas, self.eps, self.mm = lr, weight_decay, betas, eps, mm
        self.main_alpha, self.aux_alpha = main_alpha, aux_alpha
        self.accum = max(1, int(accumulation_steps))
        self.pg = process_group
        self.comm = None                 # optional comm.NativeComm: the flat-gradient all-reduce through mhimx_comm_allreduce (C-ABI) instead
        self.world = torch.distributed.get_world_size(process_group) if self._dist() else 1
        self.model_kind = model
        # data parallel, one bag per rank per update, single-pass ABMIL step: the queries' EMA is chained over the ranks (QueryChain)
        self._chain, self._chain_tokens, self._q_scratch = None, None, None
        # Participation is a property of the MODEL (ABMIL baseline with Merge), never of a bag: every path an ABMIL step can take - the
        # single-pass step, the generic step of a small / odd-shaped bag, a bag with no rows to merge - leaves this rank's tokens for the
        # chain (forward_backward raises if one did not), so that no two ranks finish an update with different formulas
        if (self.world > 1 and self.accum == 1 and model == "mhim" and student.merge_enable and student.baseline == "attn"
                and "merge.global_q_mm" in self.flat.offsets):
            rank = torch.distributed.get_rank(process_group)
            self._chain = QueryChain(self.flat.offsets["merge.global_q_mm"], student.merge.global_q_mm.numel(), float(student.merge.g_q_mm),
                                     self.world, rank)
        self._micro = 0
        self.last = {}
        dev = self.flat.student.device
        # device-resident counters: hipGraph replays freeze kernel arguments, so the dropout stream position and the
        # Adam step count live in HBM and are advanced by one-thread kernels that are part of the captured step
        self.tick = torch.zeros(1, dtype=torch.int64, device=dev)
        self.opt_step = torch.zeros(1, dtype=torch.int64, device=dev)
        self._defer = ops.ReduceList()                 # final gradient reductions of a step, flushed as one launch
        # data parallel: the flat gradient is all-reduced in two pieces, [projection weight + bias | everything else + tail]; the
        # second piece is final before the backward's longest kernel and its all-reduce overlaps it (eager steps only)
        self.overlap_comm = True
        self._work_a = None
        self._capturing = False
        fo = self.flat.offsets
        self._split = fo["feature.0.bias"] + (student.feature[0].bias.numel() + 3) // 4 * 4 if "feature.0.bias" in fo else 0
        if not (self.flat.names[:2] == ["feature.0.weight", "feature.0.bias"]):
            self._split = 0                            # unexpected parameter order: one all-reduce of the whole buffer
        student._tick = self.tick
        if teacher is not None:
            teacher._tick = self.tick
        # optional EMA-momentum schedule (one value per optimiser step): a device table indexed by the device-resident step
        # counter, so it also advances under hipGraph replay
        self.mm_table = None if mm_sche is None else torch.as_tensor(mm_sche, dtype=torch.float32).to(dev).contiguous()
        # --clip_grad (base_engine.py:115-119: clip_grad_norm_ on the accumulated gradient right before optimizer.step) and a per-update
        # learning-rate schedule (train_utils.py:69-77, base_engine.py:152-153: scheduler.step() once per update): one value per update in a
        # device table read by the optimiser kernel at the device step counter - both keep working under hipGraph replay
        self.clip_grad = None if clip_grad is None else float(clip_grad)
        self.lr_table = None if lr_sche is None else torch.as_tensor(lr_sche, dtype=torch.float32).to(dev).contiguous()
        self._clip_ws = torch.empty(1024, device=dev) if self.clip_grad else None
        self._g_extra = None
        self._fold_now, self._fold_list = False, None      # (train_step: the backward's last reductions inside the update kernel)
        self._graph_pool = None
        self._cap_stream = None
        self._side = None                  # the step executor's second stream (mhimx_step_cfg.side_stream: the step as a DAG), made on first use
        # (off by default: measured slower - every fork / join between two queues of a hipGraph costs 5-13 us, profiles/r06_dag.md)
        self.step_dag = os.environ.get("MHIMX_STEP_DAG", "0") != "0"
        # the whole step as ONE C call (mhimx_step_run, csrc/step.hip): the same launches as _forward_backward_nat + _apply, enqueued by the
        # library itself - a bag costs one ctypes call instead of ~1700 interpreter calls (the eager step was host-bound).  MHIMX_STEP_EXEC=0:
        # the Python orchestration (kept: it is the executor's specification and takes every case the executor refuses)
        self.use_executor = os.environ.get("MHIMX_STEP_EXEC", "1") != "0"
        self.wgrad_form = 0                # mhimx_step_cfg.wgrad_form: which weight-gradient kernel the step executor launches (tests force 1 / 2)
        self._exec, self.time_project = None, False      # (mhimx_step_cfg.time_project: eager steps time their projection launch - bench.py)
        self.exec_max_rows = 262144        # include/mhimx.h MHIMX_STEP_MAX_ROWS
        self.single_pass = True            # ABMIL: one projection launch for teacher + student, bag-ordered buffers (when shapes allow)
        self.window_streams = 4            # accumulation windows (window_step): HIP streams the window's bags are issued on
        # (round 6) a window of same-shaped bags as ONE C call with every launch over all its bags (mhimx_window_run, csrc/step.hip);
        # MHIMX_WINDOW_BATCHED=0: the bags on HIP streams, as rounds 3-5 had it
        self.window_batched = _WINDOW_BATCHED
        # made on first use: the stream form's side streams and slabs, its EMA weights per window length, shape_cached's graphs and counts
        self._win, self._win_w, self._shape_graphs = None, {}, None
        self._rows_cache = {}
        # 'mhim_pure' accumulation windows as ONE call (mhimx_pure_window_run): rows of the call's row space (every bag rounded up to a
        # multiple of 32) a window may have - its workspace takes 5.7 KB per row (1.5 GB at this cap); include/mhimx.h allows twice as many
        self.pure_window_row_cap = 262144
        # 'mhim' accumulation windows of different-sized bags as ONE call (mhimx_ragged_window_run): rows of the call's row space (every
        # bag's N + merge_k rounded up to a multiple of 32) a window may have - its workspace takes 7.3 KB per row (1.9 GB at this cap);
        # include/mhimx.h allows twice as many
        self.ragged_window_row_cap = 262144
        # 'mhim_pure' DSMIL steps and accumulation windows as ONE call (mhimx_dsmil_window_run): rows of the call's row space a call may
        # have - its workspace takes 9.9 KB per row (1.3 GB at this cap); include/mhimx.h allows twice as many
        self.dsmil_window_row_cap = 131072
        self._dsmil_exec = None
        # 'mhim' DSMIL steps and accumulation windows as ONE call (mhimx_dsmil_mhim_window_run): rows of the call's bag space a call may
        # have - its workspace takes 17 KB per row at the default ratios (2.2 GB at this cap, which is include/mhimx.h's)
        self.dsmil_mhim_window_row_cap = 131072
        self._dsmil_mhim_exec = None

    def _dist(self):
        return torch.distributed.is_available() and torch.distributed.is_initialized()

    @contextlib.contextmanager
    def _merge_off_if_pure(self):
        """'mhim_pure': the student runs with its Merge switched off inside the block, and gets its switch back behind it."""
        s, merge_on = self.s, self.s.merge_enable
        if self.model_kind != "mhim":
            s.merge_enable = False
        try:
            yield
        finally:
            s.merge_enable = merge_on

    def _head(self, z, teacher_feat, label, gv, accumulate):
        """The head of a bag on the Python routes: predictor, loss (cross entropy, or _surv_head), distillation and their gradients into
        ``gv``'s predictor views.  Returns (logits, losses, g_z)."""
        s = self.s
        t_in = teacher_feat.view(-1) if (teacher_feat is not None and self.aux_alpha != 0.) else None
        logits, losses, g_z, _, _ = (self._surv_head if self.loss == "nll_surv" else ops.head_fwd_bwd)(
            z, t_in, s.predictor.weight.data, s.predictor.bias.data, label, temp_t=float(s.temp_t),
            main_alpha=self.main_alpha, aux_alpha=self.aux_alpha, inv_accum=1.0 / self.accum,
            d_wp=gv["predictor.weight"], d_bp=gv["predictor.bias"], accumulate=accumulate)
        return logits, losses, g_z

    def _overlap_hook(self, first):
        """_mid_hook when this bag's backward overlaps the all-reduce of its gradient's second piece (data parallel, eager, one bag per
        update, ``first``: the update's first bag), else None."""
        return self._mid_hook if (first and self.overlap_comm and self.comm is None and self.world > 1 and self.accum == 1
                                  and not self._capturing and self._split > 0) else None

    # -------------------------------------------------------------------------------------------------
    def forward_backward(self, bag, label, perm=None, ids_shuffle=None, i=None):
        """Teacher fwd + select + student fwd + head + backward into the flat gradient buffer (accumulating).
        The native one-call routes (mhimx_step_run, mhimx_pure_step_run, mhimx_dsmil_window_run, mhimx_dsmil_mhim_window_run) take ``label``
        as an int64 tensor of one element on the bag's device; an int or a CPU label takes the Python orchestration (``self.last["exec"]``
        says which ran)."""
        x = self.s._check_x(bag)
        if self.loss == "nll_surv":
            label = self._surv_label(label, x.device)
        r = self._step_route(x, label, i, perm, ids_shuffle)
        if r.fam is not None:
            out = self._run_native(r.fam, [x], r.labels, i, bool(self._fold_now), surv=r.surv, single=True)
            return out[0][0], out[1][0]
        if r.name == "exec":
            return self._exec_step(x, label, i)
        return (self._forward_backward_nat if r.name == "nat" else self._forward_backward_py)(x, label, perm, ids_shuffle, i)

    def _step_route(self, x, label, i, perm, ids_shuffle, executor=True):
        """The _StepRoute that takes the widened bag ``x`` (``label`` of a survival trainer: _surv_label's pair): the one decision of
        forward_backward, run_steps and shape_cached, made - like _window_route's - before any seed is drawn, counter touched, workspace
        made or self.last written.  ``executor`` False: "exec" is not told from "nat" (_exec_ok is not asked).  DESIGN.md has the routes."""
        surv = self.loss == "nll_surv"
        if self.accum == 1 and perm is None and ids_shuffle is None:
            # one bag as a window of one (``x`` is the widened form already: a half bag is not offered as it is).  A survival bag (the plain
            # ABMIL student's, by the constructor): mhimx_pure_window_run_surv / mhimx_ragged_window_run_surv (accumulation_steps == 1: only the
            # orchestrations scale a bag by 1 / accumulation_steps); else the DSMIL steps: mhimx_dsmil_window_run, mhimx_dsmil_mhim_window_run
            labels, flags = ([label[0]], [label[1]]) if surv else ([label], None)
            for fam in (_PURE, _RAGGED) if surv else (_DSMIL, _DSMIL_MHIM):
                if self._native_form(fam, [x], labels, i, wide=[x]) is not None:
                    return _StepRoute(fam.run, fam, labels, flags)
        nat = self._nat_ok(x, i)
        name = "py" if not nat else "exec" if executor and self._exec_ok(x, i, perm, ids_shuffle, nat=nat) else "nat"
        return _StepRoute(name, None, label, None)

    def _forward_backward_py(self, x, label, perm, ids_shuffle, i):
        """The Python orchestration of a step: every model and every case the native calls and the single-pass step refuse."""
        s, t, fl = self.s, self.t, self.flat
        # parameter-only preparation of the step: weight transposes, paired-plane weights, query snapshot
        # (kept on the launch stream: a parallel branch in the captured hipGraph costs ~60 us of cross-queue signalling on
        # ROCm 7.2 — measured, profiles/ r01 notes — against ~40 us of kernels it would hide)
        # together with the two device counters (dropout stream position, Adam step) it is ONE launch
        prep_s = prep_t = None
        jobs = [(ops.PREP_TICK, None, self.tick)]
        if self._micro == 0:
            jobs.append((ops.PREP_TICK, None, self.opt_step))
        if s.baseline == "attn":
            if self.model_kind == "mhim":
                jt, prep_t = t.prep_jobs(backward=False)
                jobs += jt
            js, prep_s = s.prep_jobs(backward=True)
            jobs += js
        if s.baseline == "selfattn" and _STEP_IMAGES and x.shape[0] >= 2048:
            # TransMIL: the 12 weight images of the step (to_qkv / to_out of both layers: teacher and student as stored, the student's
            # also transposed for the data gradients) in this launch instead of 13 pair + 4 transpose launches along the step
            table = {}
            for model, backward in ((t if self.model_kind == "mhim" else None, False), (s, True)):
                if model is None:
                    continue
                for layer in (model.online_encoder.layer1, model.online_encoder.layer2):
                    for w in (layer.attn.to_qkv.weight.data, layer.attn.to_out[0].weight.data):
                        img = torch.empty_like(w)
                        jobs.append((ops.PREP_PAIR, w, img))
                        table[(w.data_ptr(), False)] = img
                        if backward:
                            img_t = torch.empty((w.shape[1], w.shape[0]), device=w.device)
                            jobs.append((ops.PREP_PAIR_T, w, img_t))
                            table[(w.data_ptr(), True)] = img_t
            ops.step_images(table)
        # one bf16 hi/lo image of the bag for both projections: it depends on nothing either, so it rides in the same launch
        xp = None
        if s.baseline == "attn" and s._pairable(x):
            xp = torch.empty_like(x)
            jobs.append((ops.PREP_PAIR, x, xp))
        ops.prep_batch(jobs)
        ps = x.shape[0]
        first = self._micro == 0
        gv = fl.grad_views
        if self.model_kind == "mhim":
            pre, seed_s = None, None
            if (self.single_pass and s.baseline in ("selfattn", "dsmil") and s.single_projection_ok(x) and t.single_projection_ok(x)
                    and s.act == t.act):
                # TransMIL / DSMIL: teacher AND student feature rows of all N bag rows in ONE pass over the raw bag (the reference's
                # student projects every row before it masks, mhim.py:335-336); the student's token rows are a gather, its projection
                # gradient the matrix-core-image pair on (d tokens, d out / d pre in fp16)
                tok_t = None
                if s.baseline == "selfattn":                 # the teacher's rows land under a free first row: [cls ; rows] without a copy
                    tok_t = torch.empty((1 + x.shape[0], t.feature[0].weight.shape[0]), device=x.device)
                heads = [ops.ProjHead(ops.pair_planes(t.feature[0].weight.data), t.feature[0].bias.data,
                                      drop_p=t.dropout_p if t.training else 0.0, drop_seed=t._next_seed(teacher=True),
                                      out=None if tok_t is None else tok_t[1:]),
                         None]
                seed_s = s._next_seed()
                heads[1] = ops.ProjHead(ops.pair_planes(s.feature[0].weight.data), s.feature[0].bias.data, drop_p=s.dropout_p,
                                        drop_seed=seed_s, want_dact=True)
                ops.bag_project(x, heads, act=mh.L.act_code(s.act, mh._FEATURE_ACTS), drop_tick=self.tick)
                pre = (heads[1].out, heads[1].dact)
                teacher_feat, score = t.forward_teacher(x, H=heads[0].out, tok_full=tok_t)
            else:
                teacher_feat, score = t.forward_teacher(x, xp=xp, w1p=None if prep_t is None else prep_t["w1p"],
                                                        wa_frag=None if prep_t is None else prep_t.get("wa_frag"))
            mf = s.baseline == "attn"                       # [merge | stay] rows: the pool reads [stay | merged tokens] contiguously
            rows, len_keep, Lk, R = s.student_rows(ps, i, score, perm=perm, ids_shuffle=ids_shuffle, merge_first=mf)
            plan = BagPlan(rows=rows, L=len_keep, Lk=Lk, R=R, drop_seed=s._next_seed() if seed_s is None else seed_s,
                           mca_seed=s._next_seed(), training=True, merge_first=mf)
            plan.pre = pre
            if self._chain is not None:                     # data parallel: the queries stay q0 until the update (QueryChain)
                if self._q_scratch is None:
                    self._q_scratch = torch.empty((s.merge.k, s.mlp_dim), device=x.device)
                plan.q_out = self._q_scratch
            keep_num = Lk + s.merge.k
        else:
            teacher_feat = None
            plan = s._plan_all_rows(ps)
            plan.training = True
            keep_num = ps
        if s.baseline == "selfattn":
            return self._selfattn_forward_backward(x, label, plan, teacher_feat, keep_num, first)
        if s.baseline == "dsmil":
            return self._dsmil_forward_backward(x, label, plan, teacher_feat, keep_num)
        with self._merge_off_if_pure():
            z, saved = s._bag_forward(x, plan, xp=xp, prep=prep_s)
            if self._chain is not None and self.model_kind == "mhim":
                # this rank's term of the chain: the tokens its Merge produced; a bag with no rows to merge leaves the queries alone in the
                # reference (its EMA step is skipped) - handing the chain the current queries does the same up to second order in 1 - mm
                tok = saved.get("z_tok")
                self._chain.tokens = self._chain_tokens = tok if tok is not None else s.merge.global_q_mm.data.view(s.merge.k, -1).clone()
            logits, losses, g_z = self._head(z, teacher_feat, label, gv, accumulate=not first)
            if first:
                # the six final gradient reductions of the backward (slab sums, column partials) run as ONE launch
                s._bag_backward(x, plan, saved, g_z, out=gv, defer=self._defer, mid_hook=self._overlap_hook(True))
                ops.reduce_flush(self._defer)
            else:                                   # gradient accumulation: fresh buffers, then add (rare path)
                g = s._bag_backward(x, plan, saved, g_z)
                for n, v in g.items():
                    gv[n].add_(v)
        self._micro += 1
        self.last = {"logits": logits, "losses": losses, "patch_num": ps, "keep_num": keep_num, "exec": False}
        if self.loss == "nll_surv":
            self.last["risk"] = self._risk_now
        return logits, losses

    # ------------------------------------------------------------------------------------------------- survival training (loss="nll_surv")
    @staticmethod
    def _surv_label(label, dev):
        """A survival label: the pair (Y, c) - time bin int64 [1], censorship flag fp32 [1] - as contiguous tensors on the bag's device."""
        ok = isinstance(label, (tuple, list)) and len(label) == 2 and all(torch.is_tensor(v) and v.is_cuda and v.device == dev
                                                                          and v.numel() == 1 and v.is_contiguous() for v in label)
        if not (ok and label[0].dtype == torch.int64 and label[1].dtype == torch.float32):
            raise mh.L.MhimxError(f"loss='nll_surv': a label is a pair (Y, c) - an int64 [1] time bin and an fp32 [1] censorship flag on "
                                  f"the bag's device ({dev})")
        return label[0].view(1), label[1].view(1)

    def _surv_head(self, z, t, wp, bp, label, temp_t=1.0, main_alpha=1.0, aux_alpha=0.0, inv_accum=1.0, d_wp=None, d_bp=None,
                   accumulate=False):
        """ops.head_fwd_bwd's place on the bag-after-bag route: the predictor (its label-free form: logits and the distillation loss),
        ops.surv_nll on those logits with g_scale = main_alpha * inv_accum (the fp32 product the native head takes), then
        mhimx_head_fwd_bwd's autograd form on that gradient row - the two-launch composition the native head is tested against."""
        Y, c = label
        logits, _, _, _, _ = ops.head_fwd_bwd(z, t, wp, bp, None, temp_t=temp_t, main_alpha=main_alpha, aux_alpha=aux_alpha, inv_accum=inv_accum)
        g_scale = float(torch.tensor(main_alpha, dtype=torch.float32) * torch.tensor(inv_accum, dtype=torch.float32))
        risk, nll, g = ops.surv_nll(logits.view(1, -1), Y, c, alpha=self.surv_alpha, eps=self.surv_eps, g_scale=g_scale)
        logits, ls, g_z, d_wp, d_bp = ops.head_fwd_bwd(z, t, wp, bp, None, temp_t=temp_t, main_alpha=main_alpha, aux_alpha=aux_alpha,
                                                       inv_accum=inv_accum, d_wp=d_wp, d_bp=d_bp, accumulate=accumulate, g_logits_in=g.view(-1))
        losses = torch.stack([main_alpha * nll[0] + ls[0], nll[0], ls[2]])
        self._risk_now = risk
        return logits, losses, g_z, d_wp, d_bp

    def _nat_ok(self, x, i=None):
        """True when the bag takes the single-pass ABMIL step (_forward_backward_nat): no host read-back anywhere, fixed launch shapes."""
        s, t = self.s, self.t
        return bool(self.single_pass and s.baseline == "attn" and s.bag_ordered_ok(x) and (self.model_kind != "mhim" or (
            t is not None and t.bag_ordered_ok(x) and not t.merge_test and s.merge_enable and s.v2_counts(x.shape[0], i) is not None)))

    # ------------------------------------------------------------------------------------------------- the step behind the C-ABI
    def _exec_ok(self, x, i=None, perm=None, ids_shuffle=None, window=False, nat=None):
        """True when mhimx_step_run takes this bag's step: the single-pass ABMIL step with device-drawn subsets, one process, one bag per
        update, no injected draws (csrc/step.hip: check_cfg).  ``window``: as a bag of mhimx_window_run (several bags per update).  The
        executor enqueues _forward_backward_nat's launches, so it asks _nat_ok itself (``nat``: its answer, if the caller has it): never an error."""
        s = self.s
        if ops.KERNEL_EVENT_HOOK is not None or not (self._nat_ok(x, i) if nat is None else nat):      # (the hook: events around single launches)
            return False
        if self.loss != "ce" and not window:           # (the single-bag executors have no survival form: a bag is a window of one)
            return False
        # (round 6) a data-parallel rank takes it too - forward + backward with update = 0, the EMA of the global queries sent to the
        # QueryChain's scratch (mhimx_step_cfg.q_out), then the all-reduce and mhimx_optim_step as always - unless the eager step overlaps
        # its all-reduce with the backward (the mid-backward hook lives in the Python orchestration)
        hooked = self._overlap_hook(True) is not None
        if self.model_kind == "mhim_pure":
            # mhimx_pure_step_run.  Decided on the model's kind, baseline and scorer form BEFORE anything of s.merge or
            # attention.attention[...] is touched: a pure model is built with merge_enable=False (s.merge is an Identity) and may be gated,
            # TransMIL or DSMIL.  Accumulation windows, clipping, injected draws and prec="f32" keep the Python orchestration.
            if not (self.use_executor and self.accum == 1 and not window and not hooked and not self.clip_grad and perm is None
                    and ids_shuffle is None and s.training and s.baseline == "attn" and not s.online_encoder.gated and s._op_prec != "f32"
                    and s._feature_prec(x.shape[0]) == "bf16x3" and x.dim() == 2):
                return False
            return self.pure_exec_shapes_ok(x.shape[0], x.shape[1], x.stride(0), x.stride(1), x.data_ptr(), E=s.mlp_dim,
                                            A=s.online_encoder.attention.attention[0].weight.shape[0], C=s.n_classes, max_rows=self.exec_max_rows)
        mg = s.merge                                   # (_nat_ok: the plain ABMIL student with Merge on and the v2 recipe's counts)
        if not (self.use_executor and (self.accum == 1 or window) and not hooked and perm is None and ids_shuffle is None and s.training
                and s._op_prec != "f32" and mg.attn.to_q.weight.shape[0] == 512 and mg.attn.to_kv.weight.shape[0] == 1024):
            return False
        # up to 16 384 rows: both random subsets drawn inside the one-workgroup select (MHIM.device_draw_ok: _step_counts_ok's 4096); above
        # (round 6): the multi-workgroup select with the draws as keyed permutations - the launches MHIM.student_rows issues for such bags
        c = s.v2_counts(x.shape[0], i)
        return self.step_exec_shapes_ok(x.shape[0], x.shape[1], x.stride(0), x.stride(1), x.data_ptr(), c, mg.k, E=s.mlp_dim,
                                        A=s.online_encoder.attention.attention[0].weight.shape[0], C=s.n_classes, max_rows=self.exec_max_rows)

    @staticmethod
    def _step_counts_ok(N, cnt, max_rows):
        """csrc/step.hip check_cfg's rule for a bag's row count and its (k_top, n_sel, len_keep, Lk, R)."""
        k_top, n_sel, len_keep, Lk, R = cnt
        return bool(64 <= N <= max_rows and 1 <= k_top <= (4096 if N <= 16384 else 16384) and 1 <= n_sel <= k_top
                    and len_keep == N - n_sel and Lk >= 1 and 1 <= R <= 32768 and Lk + R == len_keep)

    @staticmethod
    def step_exec_shapes_ok(N, D, pitch, inner, ptr, counts, k, E=512, A=128, C=2, max_rows=262144):
        """The tensor-free part of _exec_ok's mhim branch - csrc/step.hip check_cfg and mhimx_step_run's own argument checks, mirrored: a
        bag the call would refuse takes the Python path instead of raising.  (N, D): the bag's shape; pitch, inner: its
        strides in floats; ptr: its address; counts: its (k_top, n_sel, len_keep, Lk, R); k: merge_k."""
        return bool(ops.model_dims_ok(E, A, C, D) and 1 <= k and 8 * k <= 48 and FusedTrainer._step_counts_ok(N, counts, max_rows)
                    and ops.bag_rows_ok(N, D, pitch, inner, ptr, 4, 0, True))

    @staticmethod
    def pure_exec_shapes_ok(N, D, pitch, inner, ptr, E=512, A=128, C=2, max_rows=262144):
        """The tensor-free part of _exec_ok's pure branch - csrc/step.hip check_pure_cfg and mhimx_pure_step_run's own argument checks,
        mirrored: a bag the call would refuse takes the Python path instead of raising.  (N, D): the bag's shape; pitch, inner: its strides
        in floats; ptr: its address."""
        return bool(ops.model_dims_ok(E, A, C, D) and 64 <= N <= max_rows and ops.bag_rows_ok(N, D, pitch, inner, ptr, 4, 0, True))

    @staticmethod
    def pure_window_shapes_ok(bags, D, E=512, A=128, C=2, max_rows=262144, row_cap=524288, max_bags=32, elem=4):
        """csrc/pure_window.hip check_pw and mhimx_pure_window_run_x's own argument checks, mirrored and tensor-free: a window the call would
        refuse takes the bag-after-bag route instead of raising.  ``bags``: one (N, D, pitch, inner, ptr) per bag - shape, strides in
        elements, address; ``D``: the model's input width; ``elem``: bytes of an element of the bags' rows (4: fp32; 2: fp16 / bf16, whose
        pitch is a multiple of 8 elements and at most 2^20)."""
        return FusedTrainer._window_rows_ok(bags, D, ops.model_dims_ok(E, A, C, D), max_rows, row_cap, max_bags, elem)

    @staticmethod
    def _window_rows_ok(bags, D, model_ok, max_rows, row_cap, max_bags, elem, k=None, n_in_counts=False):
        """The row loop of the four *_window_shapes_ok.  ``model_ok``: the call's model rule; ``k``: merge_k of a full-model call, whose
        bags carry their counts behind the address (None: the teacher-free calls); ``n_in_counts``: mhimx_ragged_window_run_x - the count
        rule alone bounds a bag's rows (check_cfg) and a bag's slot holds its k tokens too."""
        if not (model_ok and D <= (1 << 20) and (k is None or (k >= 1 and 8 * k <= 48)) and 1 <= len(bags) <= max_bags):
            return False
        rows = 0
        for N, Db, pitch, inner, ptr, *cnt in bags:
            if not (Db == D and ops.bag_rows_ok(N, D, pitch, inner, ptr, elem, 0 if n_in_counts else max_rows, True)):
                return False
            if k is not None and not (cnt[0] is not None and FusedTrainer._step_counts_ok(N, cnt[0], max_rows)):
                return False
            rows += (N + (k if n_in_counts else 0) + 31) // 32 * 32
        return rows <= row_cap

    def _family_ok(self, fam, xs, labels, i=None):
        """The four _*_window_ok: True when ``fam``'s call takes these bags (fp32 bags, or fp16 / bf16 bags of ONE dtype) as one update.
        Decided before any seed is drawn or counter touched."""
        s = self.s
        if ops.KERNEL_EVENT_HOOK is not None or not xs:       # (a caller brackets single launches with events: only the Python orchestration can)
            return False
        if not (self.model_kind == fam.model_kind and s.baseline == fam.baseline and self.use_executor and self.world == 1
                and self._micro == 0 and s._op_prec != "f32" and len(labels) == len(xs) and fam.trainer_ok(self, len(xs))):
            return False
        dev, any_prec = xs[0].device, not fam.feature_bf16x3
        if not all(torch.is_tensor(x) and x.is_cuda and x.dtype == xs[0].dtype and x.dim() == 2 and x.device == dev
                   and (any_prec or s._feature_prec(x.shape[0]) == "bf16x3") for x in xs) or xs[0].dtype not in ops._X_DTYPES:
            return False
        if not ops.window_labels_ok(labels, dev):
            return False
        if fam.bags_ok is not None and not fam.bags_ok(self, xs, i, dev):
            return False
        bags = [(x.shape[0], x.shape[1], x.stride(0), x.stride(1), x.data_ptr()) + ((s.v2_counts(x.shape[0], i),) if fam.full else ())
                for x in xs]
        # (the scorer's width of an ABMIL student; a DSMIL student's q network: _dsmil_params_ok has held it to 128)
        kw = {"A": s.online_encoder.attention.attention[0].weight.shape[0]} if fam.baseline == "attn" else {"Q": 128}
        if fam.full:
            kw["k"] = s.merge.k
        max_bags = fam.max_bags if not fam.accum_caps_bags else min(self.accum, fam.max_bags) if self.accum > 1 else 1
        return getattr(self, fam.shapes)(
            bags, s.input_dim, E=s.mlp_dim, C=s.n_classes, max_rows=self.exec_max_rows, max_bags=max_bags, elem=xs[0].element_size(),
            row_cap=min(getattr(self, fam.row_cap), fam.max_rows), **kw)

    def _run_family(self, fam, xs, labels, i, update, surv=None, single=False):
        """The four _exec_*_window: one update over 1 .. accumulation_steps bags of any row counts, every loss scaled by 1 / len(bags), as
        ONE call of ``fam``'s entry point.  Returns ([logits per bag], [losses per bag]); self.last keeps the layout, the workspace and
        every bag's views.  ``surv``: the bags' censorship flags - the call's _surv form, ``labels`` are the time bins; ``single``: the one
        bag of forward_backward / train_step with the single-bag bookkeeping.  The layout call comes first: a window it refuses leaves
        every seed stream and counter alone.  Seeds are drawn bag after bag - a teacher-free bag: the feature dropout's; a full-model bag:
        _step_seeds, the order the bag-after-bag and stream routes draw them in for such a window."""
        s, fl = self.s, self.flat
        n, dev = len(xs), xs[0].device
        ex = getattr(self, fam.cfg)()
        if fam.full:
            table = (mh.L.RaggedWindowBag * n)()
            for j, (x, l) in enumerate(zip(xs, labels)):
                k_top, n_sel, len_keep, Lk, R = s.v2_counts(x.shape[0], i)
                table[j].X, table[j].ldx, table[j].N, table[j].label_dev = x.data_ptr(), x.stride(0), x.shape[0], l.data_ptr()
                table[j].cnt = mh.L.StepCounts(k_top=k_top, n_sel=n_sel, len_keep=len_keep, Lk=Lk, R=R)
        else:
            table = fam.table(xs, labels, [0] * n)
        lay = fam.layout_of(ex["cfg"], table, n)
        ws = ops.workspace(ex, fam.ws_key, lay.total, dev)
        for j in range(n):
            if fam.full:
                table[j].seeds = self._step_seeds()
            else:
                table[j].drop_seed = s._next_seed()
        inside = bool(update and not self.clip_grad)                # (clipping needs the norm of the final gradient: the update stays outside)
        risk = None if surv is None else torch.empty(n, device=dev)
        spec = None if surv is None else ops.surv_spec(surv, self.surv_alpha, self.surv_eps, risk)
        fam.call(ex["cfg"], table, n, fl.step + int(inside), ws, inside, x_dtype=ops.x_dtype_of(xs), **({} if surv is None else {"surv": spec}))
        per = fam.views(self, ws, lay, xs, table)
        logits, losses = [p["logits"] for p in per], [p["losses"] for p in per]
        if fam.full:
            self.last = dict(per[-1], logits=logits, losses=losses, bags=per, layout=lay, table=table, ws=ws, exec=fam.exec, x_dtype=xs[0].dtype)
        else:
            self.last = dict(self._last_pure(logits, losses, per[-1]["H_student"]), bags=per, layout=lay, ws=ws, exec=fam.exec, x_dtype=xs[0].dtype)
        if surv is not None:
            self.last.update(exec=fam.exec_surv, risk=risk)
        if single:
            self.last.update(logits=logits[0], losses=losses[0])
            self._steps_done(inside)
        else:
            self._window_done(n, inside, update)
        return logits, losses

    def _native_form(self, fam, bags, labels, i, offer=None, wide=None):
        """The bags in the form ``fam``'s check takes them in, or None: first as they are when all are fp16, or all bf16 (_half_bags: the
        call reads them where they lie), then widened to fp32 as every other route reads them.  ``offer`` (bags, widened) -> False: this
        form of the window is not offered to the call.  ``wide``: the caller's list of the widened bags - filled here when it is empty and
        they are needed, so that a window is widened once however many calls and routes see it.  It draws no seed and touches no counter
        or workspace (_family_ok); the check, like the call (_run_native), is looked up on the instance."""
        if self.model_kind != fam.model_kind or self.s.baseline != fam.baseline:
            return None
        ok = getattr(self, fam.ok)
        ia = (i,) if fam.full else ()
        wide = [] if wide is None else wide
        for widened in (False, True):
            if widened and not wide:
                wide.extend(self.s._check_x(b) for b in bags)
            xs = wide if widened else self._half_bags(bags)
            if xs is not None and (offer is None or offer(xs, widened)) and ok(xs, labels, *ia):
                return xs
        return None

    def _run_native(self, fam, xs, labels, i, update, surv=None, single=False):
        """``fam``'s call on the bags its check took."""
        ia = (i,) if fam.full else ()
        kw = {n: v for n, v in (("surv", surv), ("single", single)) if v}          # (only what is set: a plain window is (xs, labels[, i], update))
        return getattr(self, fam.run)(xs, labels, *ia, update, **kw)

    def _pure_window_ok(self, xs, labels):
        """True when mhimx_pure_window_run_x takes this window (_family_ok)."""
        return self._family_ok(_PURE, xs, labels)

    def _exec_pure_window(self, xs, labels, update, surv=None, single=False):
        """One accumulation window of the teacher-free model as ONE call of mhimx_pure_window_run_x / _surv (_run_family)."""
        return self._run_family(_PURE, xs, labels, None, update, surv, single)

    # ------------------------------------------------------------------------------------------------- the teacher-free DSMIL call
    _DSMIL_PARAMS = ("feature.0.weight", "feature.0.bias", "online_encoder.i_classifier.0.weight", "online_encoder.i_classifier.0.bias",
                     "online_encoder.b_classifier.q.0.weight", "online_encoder.b_classifier.q.0.bias", "online_encoder.b_classifier.q.2.weight",
                     "online_encoder.b_classifier.q.2.bias", "online_encoder.b_classifier.v.1.weight", "online_encoder.b_classifier.v.1.bias",
                     "online_encoder.b_classifier.fcc.weight", "online_encoder.b_classifier.fcc.bias")

    @staticmethod
    def dsmil_window_shapes_ok(bags, D, E=512, Q=128, C=2, max_rows=262144, row_cap=262144, max_bags=32, elem=4):
        """csrc/dsmil_window.hip check_dw and mhimx_dsmil_window_run's own argument checks, mirrored and tensor-free: a step or window the
        call would refuse takes the bag-after-bag route instead of raising.  ``bags``: one (N, D, pitch, inner, ptr) per bag - shape,
        strides in elements, address; ``D``: the model's input width; ``Q``: the q network's width; ``elem``: bytes of an element of the
        bags' rows (4: fp32; 2: fp16 / bf16, whose pitch is a multiple of 8 elements and at most 2^20)."""
        return FusedTrainer._window_rows_ok(bags, D, E == 512 and Q == 128 and 1 <= C <= 16 and D > 0 and D % 256 == 0, max_rows, row_cap,
                                            max_bags, elem)

    def _dsmil_window_ok(self, xs, labels):
        """True when mhimx_dsmil_window_run takes these bags as one update of the teacher-free DSMIL model (_family_ok)."""
        return self._family_ok(_DSMIL, xs, labels)

    def _dsmil_params_ok(self, model, dev, w1_shape=False):
        """The twelve DSMIL tensors of ``model`` as check_dw / check_dm and the kernels' 16-byte loads want them: the shapes for
        ``self.s.n_classes`` classes (``w1_shape``: feature.0.weight's too), contiguous fp32 on ``dev``, the matrices 16-byte aligned."""
        ps, Cc = model._infer_dsmil_params(), self.s.n_classes
        return bool((not w1_shape or tuple(ps[0].shape) == (512, self.s.input_dim))
                    and tuple(ps[4].shape) == (128, 512) and tuple(ps[6].shape) == (128, 128) and tuple(ps[8].shape) == (512, 512)
                    and tuple(ps[2].shape) == (Cc, 512) and ps[10].numel() == Cc * Cc * 512
                    and all(p.is_contiguous() and p.dtype == torch.float32 and p.device == dev for p in ps)
                    and not any(ps[j].data_ptr() % 16 for j in (0, 1, 2, 4, 6, 8, 9)))

    def _dsmil_base(self, b=None):
        """The mhimx_dsmil_train_cfg of this trainer - made (``b`` None: parameter / gradient pointers into the flat buffers, stable for
        the trainer's lifetime) and refreshed: the optimiser's scalars, on every call."""
        s, fl, L = self.s, self.flat, mh.L
        if b is None:
            gv = fl.grad_views
            par = L.DsmilParams(**{n: p.data_ptr() for n, p in zip(L._DSMIL_NAMES, s._infer_dsmil_params())})
            grd = L.DsmilGrads(**{n: gv[name].data_ptr() for n, name in zip(L._DSMIL_NAMES, self._DSMIL_PARAMS)})
            b = L.DsmilTrainCfg(D=s.input_dim, E=s.mlp_dim, C=s.n_classes, act=L.act_code(s.act, mh._FEATURE_ACTS), param=par, grad=grd,
                                p=fl.student.data_ptr(), g=fl.grad.data_ptr(), m=fl.m.data_ptr(), v=fl.v.data_ptr(), n_train=fl.n_train,
                                n_all=fl.n_all, tick=self.tick.data_ptr(), opt_step=self.opt_step.data_ptr())
        b.lr, b.beta1, b.beta2, b.eps, b.weight_decay = self.lr, self.betas[0], self.betas[1], self.eps, self.wd
        b.lr_table, b.lr_len = (None, 0) if self.lr_table is None else (self.lr_table.data_ptr(), self.lr_table.numel())
        b.drop_p, b.main_alpha = float(s.dropout_p), float(self.main_alpha)
        return b

    def _dsmil_cfg(self):
        """{"key", "cfg"}: the mhimx_dsmil_train_cfg of this trainer (_dsmil_base)."""
        ex = self._dsmil_exec
        key = (self.s.feature[0].weight.data_ptr(), self.flat.grad.data_ptr())
        if ex is None or ex["key"] != key:
            ex = self._dsmil_exec = {"key": key, "cfg": None}
        ex["cfg"] = self._dsmil_base(ex["cfg"])
        return ex

    def _exec_dsmil_window(self, xs, labels, update, single=False):
        """One update of the teacher-free DSMIL model as ONE call of mhimx_dsmil_window_run (_run_family)."""
        return self._run_family(_DSMIL, xs, labels, None, update, None, single)

    # ------------------------------------------------------------------------------------------------- the full MHIM(DSMIL) call
    _DSMIL_MERGE_PARAMS = ("merge.norm.weight", "merge.norm.bias", "merge.attn.to_kv.weight", "merge.attn.to_q.weight",
                           "merge.attn.to_out.0.weight", "merge.attn.to_out.0.bias")

    @staticmethod
    def dsmil_mhim_window_shapes_ok(bags, D, k, E=512, Q=128, C=2, max_rows=262144, row_cap=131072, max_bags=32, elem=4):
        """csrc/dsmil_mhim.hip check_dm and mhimx_dsmil_mhim_window_run's own argument checks, mirrored and tensor-free: a step or window
        the call would refuse takes today's route instead of raising.  ``bags``: one (N, D, pitch, inner, ptr, (k_top, n_sel, len_keep, Lk,
        R)) per bag - shape, strides in elements, address, its counts; ``D``: the model's input width; ``k``: merge_k; ``Q``: the q
        network's width; ``elem``: bytes of an element of the bags' rows (4: fp32; 2: fp16 / bf16, whose pitch is a multiple of 8 elements
        and at most 2^20)."""
        return FusedTrainer._window_rows_ok(bags, D, E == 512 and Q == 128 and 1 <= C <= 16 and D > 0 and D % 256 == 0, max_rows, row_cap,
                                            max_bags, elem, k=k)

    def _dsmil_mhim_window_ok(self, xs, labels, i=None):
        """True when mhimx_dsmil_mhim_window_run takes these bags as one update of the full MHIM(DSMIL) model: 1 .. accumulation_steps bags,
        one process, device-drawn subsets, no mid-run ratio schedule, no merge_test, no kernel event hook, not prec="f32" (_family_ok)."""
        return self._family_ok(_DSMIL_MHIM, xs, labels, i)

    def _dsmil_mhim_cfg(self):
        """The mhimx_dsmil_mhim_cfg of this trainer: parameter / gradient pointers into the flat buffers (stable for the trainer's
        lifetime); the scalars are refreshed on every call."""
        s, t, fl, L = self.s, self.t, self.flat, mh.L
        ex = self._dsmil_mhim_exec
        key = (s.feature[0].weight.data_ptr(), t.feature[0].weight.data_ptr(), fl.grad.data_ptr())
        if ex is None or ex["key"] != key:
            gv, mg = fl.grad_views, s.merge
            tea = L.DsmilParams(**{n: p.data_ptr() for n, p in zip(L._DSMIL_NAMES, t._infer_dsmil_params())})
            mps = (mg.norm.weight, mg.norm.bias, mg.attn.to_kv.weight, mg.attn.to_q.weight, mg.attn.to_out[0].weight, mg.attn.to_out[0].bias)
            mpar = L.DsmilMergeParams(**{n: p.data_ptr() for n, p in zip(L._DSMIL_MERGE_NAMES, mps)})
            mgrd = L.DsmilMergeGrads(**{n: gv[name].data_ptr() for n, name in zip(L._DSMIL_MERGE_NAMES, self._DSMIL_MERGE_PARAMS)})
            cfg = L.DsmilMhimCfg(base=self._dsmil_base(), teacher=tea, merge=mpar, merge_grad=mgrd, q=mg.global_q_mm.data_ptr(), q_out=None, k=mg.k)
            ex = self._dsmil_mhim_exec = {"key": key, "cfg": cfg}
        cfg = ex["cfg"]
        self._dsmil_base(cfg.base)
        cfg.cls_attn = int(bool(t.online_encoder.cls_attn))
        cfg.drop_p_teacher = float(t.dropout_p if t.training else 0.0)
        cfg.merge_drop_p, cfg.merge_mm = float(s.merge.dropout), float(s.merge.g_q_mm)
        cfg.temp_t, cfg.aux_alpha, cfg.ema_mm = float(s.temp_t), float(self.aux_alpha), float(self.mm)
        cfg.p_teacher = None if fl.same_teacher else fl.teacher.data_ptr()
        cfg.mm_table, cfg.mm_len = (None, 0) if self.mm_table is None else (self.mm_table.data_ptr(), self.mm_table.numel())
        return ex

    def _exec_dsmil_mhim_window(self, xs, labels, i, update, single=False):
        """One update of the full MHIM(DSMIL) model as ONE call of mhimx_dsmil_mhim_window_run (_run_family)."""
        return self._run_family(_DSMIL_MHIM, xs, labels, i, update, None, single)

    @staticmethod
    def _last_pure(logits, losses, H):
        """self.last of a teacher-free bag with the feature rows H [N, E]: no row list, no score, no tokens, no teacher."""
        N = H.shape[0]
        return {"logits": logits, "losses": losses, "patch_num": N, "keep_num": N, "rows": None, "score": None, "R": 0, "tokens": None,
                "H_student": H, "H_teacher": None}

    def _last_full(self, ws, lay, N, cnt, logits, losses, base=0, r0=0):
        """self.last of a bag of the full model: views of the workspace at the layout's offsets; ``base``: the bag's byte offset in a
        same-shape window, ``r0``: its first row in a ragged window's row space."""
        view, km, E = ops.ws_view, self.s.merge.k, self.s.mlp_dim
        Hs = view(ws, base + lay.H_student + 4 * E * r0, (N + km) * E).view(N + km, E)
        return {"logits": logits, "losses": losses, "patch_num": N, "keep_num": cnt.Lk + km,
                "rows": view(ws, base + lay.rows_all + 8 * r0, cnt.len_keep, torch.int64), "score": view(ws, base + lay.score + 4 * r0, N),
                "R": cnt.R, "tokens": Hs[N:], "H_student": Hs[:N], "H_teacher": view(ws, base + lay.H_teacher + 4 * E * r0, N * E).view(N, E)}

    def _step_seeds(self):
        """A bag's four draws in the single-bag order: both dropout streams, the select's, Merge's."""
        s, t = self.s, self.t
        return mh.L.StepSeeds(drop_teacher=t._next_seed(teacher=True), drop_student=s._next_seed(), select=s._next_seed(), mca=s._next_seed())

    def _window_done(self, n, inside, update):
        """The host's bookkeeping behind a window call of n bags: ``inside`` - the call made the update; else ``update`` makes it now."""
        self._micro = n
        if inside:
            self.flat.step += 1
            ops.step_images(None)
            self._micro = 0
        elif update:
            self.update()

    def _steps_done(self, updated, n=1):
        """Its single-bag twin, behind a call of n bags that each made their update (``updated``) or one bag that did not.  Only a step
        that was enqueued counts: a refused call leaves host and device counters equal."""
        if updated:
            self.flat.step += n
            ops.step_images(None)
            self._micro = 0
        else:
            self._micro += 1

    @staticmethod
    def _half_bags(bags):
        """The window's bags as contiguous [N, D] matrices in THEIR dtype when all of them are fp16, or all bf16, device tensors (what
        mhimx_pure_window_run_x / mhimx_ragged_window_run_x read where it lies); None for every other window."""
        if not bags or not all(torch.is_tensor(b) and b.is_cuda and b.dtype == bags[0].dtype for b in bags) \
                or bags[0].dtype not in (torch.float16, torch.bfloat16):
            return None
        xs = [b[0] if b.dim() == 3 and b.shape[0] == 1 else b for b in bags]
        return [x.contiguous() for x in xs] if all(x.dim() == 2 for x in xs) else None

    def _exec_cfg(self):
        """The mhimx_step_cfg of this trainer: parameter / gradient pointers into the flat buffers (stable for the trainer's lifetime), the
        model's hyper-parameters; the optimiser's scalars are refreshed on every call."""
        s, t, fl = self.s, self.t, self.flat
        L = mh.L
        ex = self._exec
        mhim = self.model_kind == "mhim"             # ('mhim_pure': no teacher, no merge.* fields - mhimx_pure_step_run reads neither)
        key = (s.feature[0].weight.data_ptr(), t.feature[0].weight.data_ptr() if mhim else 0, fl.grad.data_ptr())
        if ex is None or ex["key"] != key:
            P = lambda tns: tns.data_ptr()
            def params(m, with_merge):
                att = m.online_encoder.attention
                pr = L.StepParams(w1=P(m.feature[0].weight), b1=P(m.feature[0].bias), wa=P(att.attention[0].weight), wc=P(att.attention[2].weight),
                                  wp=P(m.predictor.weight), bp=P(m.predictor.bias))
                if with_merge:
                    mg = m.merge
                    pr.q, pr.ln_w, pr.ln_b = P(mg.global_q_mm), P(mg.norm.weight), P(mg.norm.bias)
                    pr.wkv, pr.wq, pr.wo, pr.bo = P(mg.attn.to_kv.weight), P(mg.attn.to_q.weight), P(mg.attn.to_out[0].weight), P(mg.attn.to_out[0].bias)
                return pr
            gv = fl.grad_views
            pre = "online_encoder.attention.attention."
            grads = L.StepGrads(w1=P(gv["feature.0.weight"]), b1=P(gv["feature.0.bias"]), wa=P(gv[pre + "0.weight"]), wc=P(gv[pre + "2.weight"]),
                                wp=P(gv["predictor.weight"]), bp=P(gv["predictor.bias"]))
            if mhim:
                grads.ln_w, grads.ln_b = P(gv["merge.norm.weight"]), P(gv["merge.norm.bias"])
                grads.wkv, grads.wq = P(gv["merge.attn.to_kv.weight"]), P(gv["merge.attn.to_q.weight"])
                grads.wo, grads.bo = P(gv["merge.attn.to_out.0.weight"]), P(gv["merge.attn.to_out.0.bias"])
            cfg = L.StepCfg(D=s.input_dim, E=s.mlp_dim, A=s.online_encoder.attention.attention[0].weight.shape[0], C=s.n_classes,
                            k=s.merge.k if mhim else 0,
                            act=L.act_code(s.act, mh._FEATURE_ACTS), da_act=L.act_code(s.da_act, mh._SCORER_ACTS),
                            student=params(s, mhim), teacher=params(t, False) if mhim else L.StepParams(), grad=grads,
                            p=P(fl.student), g=P(fl.grad), m=P(fl.m), v=P(fl.v), n_train=fl.n_train, n_all=fl.n_all,
                            tick=P(self.tick), opt_step=P(self.opt_step))
            ex = self._exec = {"key": key, "cfg": cfg, "layouts": {}, "ws": None}
        cfg = ex["cfg"]
        cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, cfg.weight_decay, cfg.ema_mm = self.lr, self.betas[0], self.betas[1], self.eps, self.wd, self.mm
        cfg.lr_table, cfg.lr_len = (None, 0) if self.lr_table is None else (self.lr_table.data_ptr(), self.lr_table.numel())
        cfg.drop_p_student = float(s.dropout_p)
        cfg.main_alpha = float(self.main_alpha)
        if not mhim:
            return ex
        if self.step_dag:
            if self._side is None or self._side.device != fl.student.device:
                self._side = torch.cuda.Stream(device=fl.student.device)
            cfg.side_stream = self._side.cuda_stream
        else:
            cfg.side_stream = None
        if self._chain is not None:                    # data parallel: the queries stay q0 until the update (QueryChain)
            if self._q_scratch is None:
                self._q_scratch = torch.empty((s.merge.k, s.mlp_dim), device=fl.student.device)
            cfg.q_out = self._q_scratch.data_ptr()
        else:
            cfg.q_out = None
        cfg.time_project = int(bool(self.time_project))
        cfg.wgrad_form = int(self.wgrad_form)
        cfg.attn2score = int(bool(t.attn2score))
        cfg.drop_p_teacher = float(t.dropout_p if t.training else 0.0)
        cfg.merge_drop_p, cfg.merge_mm = float(s.merge.dropout), float(s.merge.g_q_mm)
        cfg.temp_t, cfg.aux_alpha = float(s.temp_t), float(self.aux_alpha)
        cfg.p_teacher = None if fl.same_teacher else fl.teacher.data_ptr()
        cfg.mm_table, cfg.mm_len = (None, 0) if self.mm_table is None else (self.mm_table.data_ptr(), self.mm_table.numel())
        return ex

    def _exec_window_ok(self, xs, labels, i=None):
        """True when mhimx_window_run takes this window: 2..8 bags of ONE shape that each pass _exec_ok, up to 16 384 rows (the one-workgroup
        select), merge_k <= 6, one process, no mid-run ratio schedule (csrc/step.hip: check_window)."""
        n = len(xs)
        if not (self.window_batched and 2 <= n <= _L.WINDOW_MAX and self.world == 1 and self._chain is None and not self.step_dag
                and self.flat.n_all % 4 == 0 and self.s.merge.k <= 6 and self.s.mrh_sche is None and self.flat.names[0] == "feature.0.weight"):
            return False
        x0 = xs[0]
        if not (x0.dim() == 2 and x0.shape[0] <= 16384 and all(x.shape == x0.shape and x.stride() == x0.stride() and x.device == x0.device for x in xs)):
            return False
        if not ops.window_labels_ok(labels, x0.device):
            return False
        return all(self._exec_ok(x, i, window=True) for x in xs)

    def _exec_window(self, xs, labels, i, update):
        """One accumulation window as ONE call of mhimx_window_run: every launch between the projections and the weight gradient covers all
        the bags (include/mhimx.h).  Returns ([logits per bag], [losses per bag]); self.last["bags"] holds each bag's views."""
        L = mh.L
        s, t, fl = self.s, self.t, self.flat
        n = len(xs)
        ex = self._exec_cfg()
        N = xs[0].shape[0]
        k, n_sel, len_keep, Lk, R = s.v2_counts(N, i)
        key = ("window", n, N, k, n_sel, Lk)
        ent = ex["layouts"].get(key)
        if ent is None:
            cnt = L.StepCounts(k_top=k, n_sel=n_sel, len_keep=len_keep, Lk=Lk, R=R)
            ent = ex["layouts"][key] = (cnt, ops.window_layout(ex["cfg"], n, N, cnt))
        cnt, lay = ent
        ws = ops.workspace(ex, "ws_win", lay.total, xs[0].device, slack=1.0)      # (exactly the window's bytes: its layout is cached by shape)
        # (the order the stream form with MHIMX_WINDOW_PROJECT=1 draws them in: every bag's dropout streams at the projection, then bag
        # after bag the select's and Merge's - the two forms of a window make the same draws)
        seeds = (L.StepSeeds * n)()
        for j in range(n):
            seeds[j].drop_teacher, seeds[j].drop_student = t._next_seed(teacher=True), s._next_seed()
        for j in range(n):
            seeds[j].select, seeds[j].mca = s._next_seed(), s._next_seed()
        inside = bool(update and not self.clip_grad)              # (clipping needs the norm of the final gradient: the update stays outside)
        ops.window_run(ex["cfg"], xs, labels, cnt, seeds, fl.step + int(inside), ws, inside)
        bg = lay.bag
        per = []
        for j in range(n):
            base = j * lay.bag_stride
            per.append(self._last_full(ws, bg, N, cnt, ops.ws_view(ws, base + bg.logits, s.n_classes), ops.ws_view(ws, base + bg.losses, 3), base=base))
        logits, losses = [p["logits"] for p in per], [p["losses"] for p in per]
        self.last = dict(per[-1], logits=logits, losses=losses, bags=per, ws=ws, exec="mhimx_window_run")
        self._window_done(n, inside, update)
        return logits, losses

    # ------------------------------------------------------------------------------------------------- the ragged window behind the C-ABI
    @staticmethod
    def ragged_window_shapes_ok(bags, D, k, E=512, A=128, C=2, max_rows=262144, row_cap=524288, max_bags=32, elem=4):
        """csrc/ragged_window.hip check_rw (csrc/step.hip check_cfg per bag) and mhimx_ragged_window_run_x's own argument checks, mirrored and
        tensor-free: a window the call would refuse takes today's route instead of raising.  ``bags``: one (N, D, pitch, inner, ptr,
        (k_top, n_sel, len_keep, Lk, R)) per bag - shape, strides in elements, address, its counts; ``D``: the model's input width; ``k``:
        merge_k; ``elem``: bytes of an element of the bags' rows (4: fp32; 2: fp16 / bf16, whose pitch is a multiple of 8 elements and at
        most 2^20)."""
        return FusedTrainer._window_rows_ok(bags, D, ops.model_dims_ok(E, A, C, D), max_rows, row_cap, max_bags, elem, k=k, n_in_counts=True)

    def _ragged_window_ok(self, xs, labels, i=None):
        """True when mhimx_ragged_window_run takes this window: 1 .. accumulation_steps bags that each take the step executor, one process,
        device-drawn subsets, no mid-run ratio schedule, merge_k <= 6 (_family_ok)."""
        return self._family_ok(_RAGGED, xs, labels, i)

    def _exec_ragged_window(self, xs, labels, i, update, surv=None, single=False):
        """One accumulation window of different-sized bags as ONE call of mhimx_ragged_window_run_x / _surv (_run_family)."""
        return self._run_family(_RAGGED, xs, labels, i, update, surv, single)

    def _exec_plan(self, ex, N, i):
        """(counts, layout) of a bag of N rows at iteration i - cached: they follow from N and the HAM ratio alone."""
        pure = self.model_kind == "mhim_pure"              # (no counts: every row takes part)
        c = None if pure else self.s.v2_counts(N, i)
        key = ("pure", N) if pure else (N, c[0], c[1], c[3])
        ent = ex["layouts"].get(key)
        if ent is None:
            cnt = None if pure else mh.L.StepCounts(k_top=c[0], n_sel=c[1], len_keep=c[2], Lk=c[3], R=c[4])
            ent = ex["layouts"][key] = (cnt, ops.step_layout(ex["cfg"], N, cnt))
        return ent

    def _last_step(self, ws, lay, N, cnt):
        """self.last of a single-bag call: the bag's dictionary (``cnt`` None: the teacher-free form), the workspace, the route."""
        logits, losses = ops.ws_view(ws, lay.logits, self.s.n_classes), ops.ws_view(ws, lay.losses, 3)
        if cnt is None:
            bag = self._last_pure(logits, losses, ops.ws_view(ws, lay.H_student, N * self.s.mlp_dim).view(N, self.s.mlp_dim))
        else:
            bag = self._last_full(ws, lay, N, cnt, logits, losses)
        return dict(bag, ws=ws, exec=True)

    def _exec_step(self, x, label, i):
        """forward_backward (+ the update, inside train_step) of one bag as ONE call of mhimx_step_run ('mhim_pure': mhimx_pure_step_run)."""
        ops.check_label(label, x.device, f"label: expected a contiguous int64 tensor on the bag's device ({x.device})")
        ex = self._exec_cfg()
        N = x.shape[0]
        cnt, lay = self._exec_plan(ex, N, i)
        # a captured step owns its workspace (the graph's memory pool); eager steps share one that only grows
        ws = ops.workspace(ex, "ws", lay.total, x.device)
        # 'mhim_pure': ONE seed per bag - the feature dropout's, drawn exactly where _nat_heads draws it: the model's seed stream then
        # stands where the Python path leaves it
        seeds = self.s._next_seed() if cnt is None else self._step_seeds()
        update = bool(self._fold_now)
        ops.step_run(ex["cfg"], x, label, cnt, seeds, self.flat.step + int(update), ws, update)
        self.last = self._last_step(ws, lay, N, cnt)
        if self._chain is not None and cnt is not None:     # this rank's term of the chain: the tokens its Merge produced
            self._chain.tokens = self._chain_tokens = self.last["tokens"]
        self._steps_done(update)
        return self.last["logits"], self.last["losses"]

    def run_steps(self, bags, labels, i=None):
        """len(bags) consecutive complete train steps (one update each) as ONE call of mhimx_step_run_many (SURVEY 7 H4 "run_steps"): the
        bags of a resident dataset, bag after bag, on one workspace.  ``i``: the iteration of the FIRST bag (bag j runs at i + j, as the
        reference's loop counts them - base_engine.py:78) or a sequence with one entry per bag.  Returns the last bag's (logits, losses).
        What the executor's in-launch update does not do - clipping (base_engine.py:115-119), unfolded reductions, accumulation, the survival
        loss - and every chunk with a bag whose route (_step_route) is not "exec" goes bag by bag through train_step, which does."""
        L = mh.L
        n = len(bags)
        if n == 0 or len(labels) != n:
            raise L.MhimxError(f"run_steps: {n} bags, {len(labels)} labels")
        its = list(i) if isinstance(i, (list, tuple)) else [None if i is None else i + j for j in range(n)]
        if len(its) != n:
            raise L.MhimxError(f"run_steps: {len(its)} iteration indices for {n} bags")
        xs = [self.s._check_x(b) for b in bags]
        if self._micro != 0:
            raise L.MhimxError("run_steps: called inside an accumulation window (a fresh update is required)")
        if self.clip_grad or self.accum != 1 or self.world != 1 or self.loss != "ce" or not all(
                self._step_route(x, l, it, None, None).name == "exec" for x, l, it in zip(xs, labels, its)):
            out = None
            for b, l, it in zip(bags, labels, its):
                out = self.train_step(b, l, i=it)
            return out
        for x, l in zip(xs, labels):
            ops.check_label(l, x.device, f"run_steps: every label must be a contiguous int64 tensor on its bag's device ({x.device})", nonempty=True)
        ex = self._exec_cfg()
        plans = [self._exec_plan(ex, x.shape[0], it) for x, it in zip(xs, its)]
        ws = ops.workspace(ex, "ws", max(p[1].total for p in plans), xs[0].device)
        cnt, lay = plans[-1]
        pure = cnt is None
        seeds = [self.s._next_seed() if pure else self._step_seeds() for _ in range(n)]
        ops.step_run_many(ex["cfg"], xs, labels, None if pure else [p[0] for p in plans], seeds, self.flat.step + 1, ws)
        self._steps_done(True, n)
        last = self._last_step(ws, lay, xs[-1].shape[0], cnt)
        if pure:                                            # (the full model's run_steps leaves self.last as it found it)
            self.last = last
        return last["logits"], last["losses"]

    def _forward_backward_nat(self, x, label, perm, ids_shuffle, i):
        """The single-pass ABMIL step: ONE projection launch computes the teacher's and the student's feature rows from the raw bag
        (the reference's student projects all N rows before it masks, mhim.py:335-336); the rows stay in bag order and the scorer,
        Merge, their backwards and the projection's weight-gradient GEMM gather the rows that take part by index."""
        first = self._micro == 0
        # caller-supplied tensors are validated HERE: inside the pinned step the wrappers skip their argument checks (ops._chk)
        for tns, nm in ((label, "label"), (perm, "perm"), (ids_shuffle, "ids_shuffle")):
            if torch.is_tensor(tns) and not (tns.is_cuda and tns.dtype == torch.int64 and tns.is_contiguous() and tns.device == x.device):
                raise mh.L.MhimxError(f"{nm}: expected a contiguous int64 tensor on the bag's device ({x.device}), got {tns.dtype} on {tns.device}")
        with ops.pinned_stream():                              # (one bag, one stream: the launches' stream is looked up once)
            res = self._nat_prep([x], i, with_opt_tick=first, split=True)       # (the student-side preparation jobs ride in the teacher's scorer launch)
            prep_t, preps = res[0], res[1]
            preps[0]["_ride_jobs"] = res[2] if len(res) > 2 else None
            out = self._nat_bag(x, label, prep_t, preps[0], self.flat.grad_views, accumulate=not first, perm=perm, ids_shuffle=ids_shuffle,
                                i=i, mid_hook=self._overlap_hook(first))
        self._micro += 1
        return out

    def _nat_prep(self, xs, i, with_opt_tick=True, split=False):
        """The parameter-only preparation for the bags ``xs`` that share the current weights (one bag, or an accumulation window) as ONE
        launch: device counters, paired-plane / fragment / transposed weight images of both models, and - per bag, because it lives at the
        head of that bag's Merge workspace - the query side of the projection-free Merge.  Returns (teacher prep, [student prep per bag]).
        ``split`` (one bag, MHIM): only what the projection and the teacher's scorer read - the counters, both projection weight images,
        the teacher's scorer image - is launched here; everything else (the student's scorer images, the backward's transposes, the query
        snapshot, the Merge preparation's chain: ~2/3 of the launch's time) is returned as a third value and rides in the teacher's scorer
        launch (ops.abmil_pool_fwd(ride_jobs=)), off the head of the step's chain."""
        s, t = self.s, self.t
        mhim = self.model_kind == "mhim"
        dev = xs[0].device
        jobs = [(ops.PREP_TICK, None, self.tick)]
        if with_opt_tick:
            jobs.append((ops.PREP_TICK, None, self.opt_step))
        prep_t = None
        if mhim:
            jt, prep_t = t.prep_jobs(backward=False)
            jobs += jt
        with self._merge_off_if_pure():
            Rs = [s.v2_counts(x.shape[0], i)[4] if mhim else 0 for x in xs]
            lean = mhim and s.merge.k * 8 <= 48 and all(1 <= R <= 32768 for R in Rs) and s._op_prec != "f32"
            js, prep_s = s.prep_jobs(backward=True, lean_merge=lean)
            preps = []
            for R in Rs:
                pb = dict(prep_s)
                if lean:
                    # the parameter-only part of the student's Merge (LayerNorm of the queries, their projection, the score vectors) rides
                    # in the preparation launch: off the teacher -> select -> student chain
                    mw_prep = s._merge_w(None)
                    pb["merge_ws"] = mw_prep.ws_for(R, dev)
                    pb["_merge_prep_w"] = mw_prep                          # (keeps the weight struct alive until the launch is enqueued)
                    js.append((ops.PREP_MERGE, mw_prep, (pb["merge_ws"], R)))
                preps.append(pb)
            late = []
            if split and mhim and len(xs) == 1:
                w1_ptr = s.feature[0].weight.data_ptr()
                early = [j for j in js if j[0] == ops.PREP_PAIR and j[1].data_ptr() == w1_ptr]
                late = [j for j in js if not any(j is e for e in early)]
                js = early
            ops.prep_batch(jobs + js)
        return (prep_t, preps, late) if split else (prep_t, preps)

    def _nat_heads(self, x, prep_t, prep_s):
        """The student's feature buffer [N + k, E] (the k rows behind the bag: Merge's tokens) and both models' projection heads of a bag."""
        s, t = self.s, self.t
        mhim = self.model_kind == "mhim"
        k = s.merge.k if mhim else 0
        Hbuf = torch.empty((x.shape[0] + k, s.mlp_dim), device=x.device)
        heads = []
        if mhim:
            p_t = t.dropout_p if t.training else 0.0                # the trainer keeps the teacher in train mode
            heads.append(ops.ProjHead(prep_t["w1p"], t.feature[0].bias.data, drop_p=p_t, drop_seed=t._next_seed(teacher=True)))
        heads.append(ops.ProjHead(prep_s["w1p"], s.feature[0].bias.data, drop_p=s.dropout_p, drop_seed=s._next_seed(), out=Hbuf, want_dact=True))
        return Hbuf, heads

    def _nat_bag(self, x, label, prep_t, prep_s, gv, accumulate=False, perm=None, ids_shuffle=None, i=None, mid_hook=None, q_out=None, slot=0,
                 wgrad_park=None, projected=None):
        """One bag of the single-pass step after its preparation: projection (teacher + student), teacher pool, select, Merge, student
        pool, head, backward.  ``gv``: the gradient views to fill (``accumulate``: add to them); ``q_out``: where Merge's EMA-updated
        queries go (default: the parameter itself, merge.py:142-143)."""
        s, t = self.s, self.t
        mhim = self.model_kind == "mhim"
        ps, E = x.shape[0], s.mlp_dim
        dev = x.device
        with self._merge_off_if_pure():
            k = s.merge.k if mhim else 0
            act = mh.L.act_code(s.act, mh._FEATURE_ACTS)
            if projected is None:
                Hbuf, heads = self._nat_heads(x, prep_t, prep_s)
                ops.bag_project(x, heads, act=act, drop_tick=self.tick)
            else:                                                 # an accumulation window projected all its bags in one launch
                Hbuf, heads = projected
            DACT = heads[-1].dact
            teacher_feat, rows_all, score = None, None, None
            if mhim:
                wp = t.predictor.weight.data if t.attn2score else None
                st_t = ops.abmil_pool_fwd(t._scorer(prep_t.get("wa_frag")), heads[0].out, None, wp=wp,
                                          bp=t.predictor.bias.data if t.attn2score else None, ride_jobs=prep_s.get("_ride_jobs"), no_backward=True)
                score = st_t.pscore if t.attn2score else ops.softmax_from_stats(st_t.s, st_t.stats)
                teacher_feat = st_t.z
                _, _, len_keep, Lk, R = s.v2_counts(ps, i)
                # [rows to merge | rows that stay | the k token rows ps .. ps+k-1]
                key = (ps, len_keep, k, slot)                         # (one list per bag of a window: the bags may run concurrently)
                rows_all = self._rows_cache.get(key)
                if rows_all is None:
                    rows_all = torch.empty(len_keep + k, dtype=torch.int64, device=dev)
                    rows_all[len_keep:] = torch.arange(ps, ps + k, device=dev)
                    self._rows_cache[key] = rows_all
                s.student_rows(ps, i, score.view(1, -1), perm=perm, ids_shuffle=ids_shuffle, merge_first=True, rows_out=rows_all)
                plan = BagPlan(rows=rows_all[:len_keep], L=len_keep, Lk=Lk, R=R, mca_seed=s._next_seed(), training=True, merge_first=True)
                if q_out is None and self._chain is not None:         # data parallel: the queries stay q0 until the update (QueryChain)
                    if self._q_scratch is None:
                        self._q_scratch = torch.empty((k, E), device=dev)
                    q_out = self._q_scratch
                    self._chain.tokens = self._chain_tokens = Hbuf[ps:]
                plan.q_out = q_out
                keep_num = Lk + k
            else:
                plan = BagPlan(rows=None, L=ps, Lk=ps, R=0, training=True)
                keep_num = ps
            z, saved = s._bag_forward_nat(x, plan, Hbuf, DACT, rows_all, prep_s)
            logits, losses, g_z = self._head(z, teacher_feat, label, gv, accumulate)
            # the six final gradient reductions of the backward (slab sums, column partials) run as ONE launch
            # train_step (one bag per update, one process, no clipping): nothing reads the gradient between this backward and the update,
            # so no reduction launch stands between them - the reductions that are final before the weight-gradient product starts ride in
            # its launch (ride_tail), and the product's own split-K slab sum is folded into the update kernel (_apply: fold)
            fold = self._fold_now and not accumulate and wgrad_park is None and mid_hook is None
            s._bag_backward_nat(x, plan, saved, g_z, gv, defer=self._defer, mid_hook=mid_hook, accumulate=accumulate, wgrad_park=wgrad_park,
                                ride_tail=fold)
            if fold:
                self._fold_list = self._defer
            else:
                ops.reduce_flush(self._defer)
        # (kept for inspection / parity tests: under graph replay these are the static buffers the replay rewrites)
        self.last = {"logits": logits, "losses": losses, "patch_num": ps, "keep_num": keep_num, "rows": plan.rows,
                     "score": score, "R": plan.R, "tokens": Hbuf[ps:] if mhim else None,
                     "H_student": Hbuf[:ps], "H_teacher": heads[0].out if mhim else None, "exec": False}
        if self.loss == "nll_surv":
            self.last["risk"] = self._risk_now
        return logits, losses

    # ------------------------------------------------------------------------------------------------- accumulation windows
    def window_ok(self, bags, i=None):
        """The batched window takes the single-pass ABMIL step for every bag (_nat_ok: the shapes _forward_backward_nat takes) of the full
        model, with device-drawn subsets and the dedicated weight-gradient pair, no mid-run ratio schedule, one process."""
        s, xs = self.s, [b[0] if b.dim() == 3 else b for b in bags]
        if self.model_kind != "mhim" or not self.single_pass or s.mrh_sche is not None:
            return False
        if not all(x.is_cuda and self._nat_ok(x, i) and s.device_draw_ok(x.shape[0], i)
                   and ops.bag_wgrad_ok(x, s.mlp_dim, s.v2_counts(x.shape[0], i)[2]) for x in xs):
            return False
        return not ((_WINDOW_WGRAD or _WINDOW_PROJECT) and len({tuple(x.shape) for x in xs}) > 1)       # (they size their workspace from bag 0)

    def _window_state(self, n_streams, dev):
        """Side streams and their gradient slabs (stream 0 = the caller's stream accumulates straight into the flat gradient)."""
        st = self._win
        if st is None or len(st["streams"]) < n_streams - 1:
            fl = self.flat
            slabs = torch.zeros((max(n_streams - 1, 1), fl.n_all), device=dev)
            pd = dict(self.s.named_parameters())
            views = [{n: slabs[j, fl.offsets[n]:fl.offsets[n] + pd[n].numel()].view_as(pd[n]) for n in fl.train_names}
                     for j in range(n_streams - 1)]
            st = self._win = {"streams": [torch.cuda.Stream() for _ in range(n_streams - 1)], "slabs": slabs, "views": views,
                              "defers": [ops.ReduceList() for _ in range(n_streams - 1)]}
        return st

    def window_step(self, bags, labels, i=None, n_streams=None, perms=None, shuffles=None, update=True):
        """ONE optimiser update over ``accumulation_steps`` bags that share the current weights (--accumulation_steps,
        base_engine.py:29,47-49,100-119,146-167), as a batch instead of a loop:

        * the parameter-only preparation (weight images, Merge's query side) runs ONCE for the window, Adam + EMA once (as in the loop);
        * the k bags are independent until the gradient sum (teacher and student weights are fixed inside a window), so they are issued
          round-robin on ``n_streams`` HIP streams: bag j's latency-bound launches (select, Merge, scorers, head: one to a few dozen
          workgroups each) run beside bag j'+1's projection and weight-gradient GEMMs instead of on one serial chain.  Stream 0 (the
          caller's) accumulates into the flat gradient, every other stream into its own slab; ONE reduce launch sums the slabs;
        * Merge's in-forward EMA of the global queries (merge.py:142-143): every bag attends with the window's first queries, and the
          window ends with the same chain of EMA steps on the tokens those forwards produced (oracle ``train_window(q_ema="window")``;
          differs from the reference's bag-after-bag order in second order of 1 - merge_mm).
        Each bag's loss is scaled by 1 / accumulation_steps in the head kernel (base_engine.py:102).  Capturable (``capture_window``).
        That is the stream form (_stream_window); which windows take a native call instead, which go bag after bag, and in which order
        they are offered: _window_route, and the route table in DESIGN.md ("Native calls: the shared host pieces").
        ``self.last["exec"]`` names the route.  Returns ([logits per bag], [losses per bag])."""
        k, surv = len(bags), self.loss == "nll_surv"
        if surv:
            labels = [self._surv_label(l, bags[0].device) for l in labels]
        if surv or (self.model_kind == "mhim_pure" and self.accum > 1):
            assert 1 <= k <= self.accum and len(labels) == k, "window_step takes at most accumulation_steps bags"
        r = self._window_route(bags, labels, i, perms, shuffles)
        if r.fam is not None:
            return self._run_native(r.fam, r.xs, r.labels, i, update, surv=r.surv)
        if r.name == "bag_surv":
            return self._bag_after_bag(bags, labels, i, perms, shuffles, update=update, aggregate=True)
        if r.name == "bag":                                            # (train_step, whatever ``update`` says)
            return self._bag_after_bag(bags, labels, i, perms, shuffles, update=True, aggregate=False)
        assert k == self.accum and len(labels) == k, "window_step takes exactly accumulation_steps bags"
        assert self._micro == 0, "window_step starts a fresh accumulation window"
        if r.name == "window_run":
            return self._exec_window(r.xs, labels, i, update)
        return self._stream_window(r.xs, labels, i, n_streams, update)

    def _window_route(self, bags, labels, i, perms, shuffles):
        """The _Route that takes this window (``labels`` of a survival trainer: _surv_label's pairs): window_step's and capture_window's
        one decision, made before any seed is drawn, counter touched or workspace made.  DESIGN.md has the table in words."""
        k, pure, surv = len(bags), self.model_kind == "mhim_pure", self.loss == "nll_surv"
        Ys, censored = ([p[0] for p in labels], [p[1] for p in labels]) if surv else (labels, None)
        # the route table - offers: (family, labels, censorship flags, which forms of the window it is offered) in order, made only without
        # injected draws; rest: who takes what they refuse (None: window_ok, the draws and world decide between "bag", "window_run", "stream").
        # capture_window asks for the widened bags without draws, and accepts what _RAGGED's check takes even where ragged_too keeps the
        # window from it: with window_ok False such a window is captured bag after bag
        if surv and pure:
            offers, rest = [(_PURE, Ys, censored, None)], "bag_surv"
        elif pure and self.accum > 1:
            offers, rest = [(_DSMIL if self.s.baseline == "dsmil" else _PURE, labels, None, None)], "bag"
        else:
            # (a full window of same-shaped bags keeps mhimx_window_run, or the stream form where that call does not take it; the survival
            # trainer's second offer has the pairs as labels, which no check takes)
            ragged_too = lambda xs, widened: not (k == self.accum and all(
                x.shape == xs[0].shape and (not widened or x.stride() == xs[0].stride()) for x in xs))
            offers, rest = [(_RAGGED, Ys, censored, None)] if surv else [], None
            if 1 <= k <= self.accum:
                offers.append((_DSMIL_MHIM, labels, None, None))
            offers.append((_RAGGED, labels, None, ragged_too))
        wide = []                                                     # (the widened bags, made once: by the first offer or route that needs them)
        if perms is None and shuffles is None:
            for fam, lab, flags, offer in offers:
                xs = self._native_form(fam, bags, lab, i, offer, wide)
                if xs is not None:
                    return _Route(fam.run, fam, xs, lab, flags)
        if rest is not None:
            return _Route(rest, None, bags, labels, None)
        xs = wide or [self.s._check_x(b) for b in bags]
        if not self.window_ok(xs, i) or perms is not None or self.world > 1:
            return _Route("bag", None, bags, labels, None)
        return _Route("window_run" if self._exec_window_ok(xs, labels, i) else "stream", None, xs, labels, None)

    def _bag_after_bag(self, bags, labels, i, perms, shuffles, update, aggregate):
        """A window no call and neither window form takes: train_step (``update`` False: forward_backward) bag after bag, which scales
        by 1 / accumulation_steps and so needs exactly that many bags.  ``aggregate``: self.last gathers the bags' - "bags", "risk"."""
        assert len(bags) == self.accum and len(labels) == len(bags), "window_step takes exactly accumulation_steps bags"
        step = self.train_step if update else self.forward_backward
        outs, per = [], []
        for j, (b, l) in enumerate(zip(bags, labels)):
            outs.append(step(b, l, i=i, **({} if perms is None else {"perm": perms[j], "ids_shuffle": shuffles[j]})))
            per.append(self.last)
        logits, losses = [o[0] for o in outs], [o[1] for o in outs]
        if aggregate:
            self.last = dict(self.last, logits=logits, losses=losses, bags=per, risk=torch.cat([b["risk"].view(1) for b in per]))
        return logits, losses

    def _stream_window(self, xs, labels, i, n_streams, update):
        """window_step's stream form (its docstring): the window's bags round-robin on HIP streams, one preparation, one update."""
        k = len(xs)
        S = max(1, min(int(n_streams or self.window_streams), k))
        dev = xs[0].device
        s, fl = self.s, self.flat
        prep_t, preps = self._nat_prep(xs, i, with_opt_tick=True)
        st = self._window_state(S, dev)
        km, E = s.merge.k, s.mlp_dim
        q_new = torch.empty((k, km, E), device=dev)                   # per-bag EMA outputs (unused: the chain below runs on the tokens)
        main = torch.cuda.current_stream()
        ev0 = torch.cuda.Event()
        ev0.record(main)
        logits, losses, tokens, per_bag = [None] * k, [None] * k, [None] * k, []
        park = [] if _WINDOW_WGRAD else None                          # the bags' dPre images: ONE weight-gradient product for the window
        proj = [None] * k
        if _WINDOW_PROJECT and k <= 8:
            # both models' projections of ALL the window's bags in one launch (mhimx_bag_project_multi): the weights are the window's, a bag's
            # last row tiles drain their 51 MB of outputs under the next bag's loops, and no projection fills every CU later, in the middle
            # of the other streams' small launches
            proj = [self._nat_heads(x, prep_t, pp) for x, pp in zip(xs, preps)]
            ops.bag_project_multi(xs, [h for _, h in proj], act=mh.L.act_code(s.act, mh._FEATURE_ACTS), drop_tick=self.tick)
            ev0.record(main)                                          # (the side streams start behind the projection)
        keep_defer = self._defer
        try:
            for j in range(k):
                lane = j % S
                stream = main if lane == 0 else st["streams"][lane - 1]
                gv = fl.grad_views if lane == 0 else st["views"][lane - 1]
                if lane and j < S:
                    stream.wait_event(ev0)
                self._defer = keep_defer if lane == 0 else st["defers"][lane - 1]
                with torch.cuda.stream(stream):
                    logits[j], losses[j] = self._nat_bag(xs[j], labels[j], prep_t, preps[j], gv, accumulate=(j >= S), i=i,
                                                         q_out=q_new[j], slot=j, wgrad_park=park, projected=proj[j])
                    tokens[j] = self.last["tokens"]
                    per_bag.append(self.last)
        finally:
            self._defer = keep_defer
        for lane in range(1, S):
            e = torch.cuda.Event()
            e.record(st["streams"][lane - 1])
            main.wait_event(e)
        if park:
            # dW1 (+)= sum_bags dPre_b^T X_b as ONE launch (mhimx_bag_wgrad_multi): every bag owns its slabs of k-steps, and what a launch pays
            # once - row tables, first tiles, 34 MB of split-K slabs written and summed - is paid once per window (8 x (36 + 9) -> 236 + 16 us)
            ops.bag_wgrad_multi(park, fl.grad_views["feature.0.weight"], accumulate=False, defer=self._defer)
            ops.reduce_flush(self._defer)
        if S > 1:                                                     # the other streams' slabs: summed into the gradient by the optimiser
            if update and self.world == 1:                            # kernel itself (mhimx_optim_args.g_extra); else by one reduce launch
                self._g_extra = st["slabs"][:S - 1]
            else:
                lst = ops.ReduceList()
                ops.reduce_slabs_job(lst, st["slabs"][:S - 1], fl.grad, accumulate=True)
                ops.reduce_flush(lst)
        # the window's EMA chain on the k token sets: q <- mm^k q + (1 - mm) sum_j mm^(k-1-j) z_j
        mm = float(s.merge.g_q_mm)
        w = self._win_w.get(k)
        if w is None:                                                 # (device arithmetic only: capture-safe)
            w = self._win_w[k] = ((1.0 - mm) * mm ** torch.arange(k - 1, -1, -1, device=dev, dtype=torch.float64)).float()
        Z = torch.stack(tokens)                                       # [k, km, E]
        q = s.merge.global_q_mm.data.view(km, E)
        q.mul_(mm ** k).add_((Z * w.view(k, 1, 1)).sum(0))
        self._micro = k
        if update:
            self.update()
        self.last = dict(self.last, logits=logits, losses=losses, bags=per_bag)
        if self.loss == "nll_surv":
            self.last["risk"] = torch.cat([b["risk"].view(1) for b in per_bag])
        return logits, losses

    def capture_window(self, bags, labels, warmup=1, n_streams=None, **kw):
        """Capture one whole accumulation window (window_step) on static (bags, labels) into ONE hipGraph whose branches are the
        window's streams; ``graph.replay()`` runs prep, the k bags, the slab sum, Adam + EMA."""
        if self.world > 1:
            raise mh.L.MhimxError("capture_window: one process (data-parallel ranks exchange gradients between windows: use capture())")
        # the route of the widened bags without injected draws (_window_route says where that differs from window_step's own question)
        i, surv = kw.get("i"), self.loss == "nll_surv"
        xs = [self.s._check_x(b) for b in bags]
        r = self._window_route(xs, [self._surv_label(l, xs[0].device) for l in labels] if surv else labels, i, None, None)
        if surv or (self.model_kind == "mhim_pure" and self.accum > 1):
            if r.fam is None:
                calls = "mhimx_pure_window_run_surv / mhimx_ragged_window_run_surv" if surv else "mhimx_pure_window_run / mhimx_dsmil_window_run"
                raise mh.L.MhimxError(f"capture_window: {calls} does not take these bags / this model")
        elif r.name == "bag" and not self._ragged_window_ok(xs, labels, i):
            raise mh.L.MhimxError("capture_window: these bags / this model do not take the single-pass ABMIL step")
        step = lambda: self.window_step(bags, labels, n_streams=n_streams, **kw)
        self._capturing = True
        try:
            cs = self._capture_stream()
            self._warm_up(cs, step, warmup)
            torch.cuda.synchronize()
            return self._record(cs, step)[0]
        finally:
            self._capturing = False

    # ------------------------------------------------------------------------------------------------- graph capture: the shared steps
    def _capture_stream(self):
        """The trainer's capture stream - made on first use - behind the work the current stream holds."""
        if self._cap_stream is None:
            self._cap_stream = torch.cuda.Stream()
        self._cap_stream.wait_stream(torch.cuda.current_stream())
        return self._cap_stream

    def _warm_up(self, cs, fn, n=1):
        """``fn`` n times on the capture stream, the current stream behind it.  Returns what the last call returned."""
        out = None
        with torch.cuda.stream(cs):
            for _ in range(n):
                out = fn()
        torch.cuda.current_stream().wait_stream(cs)
        return out

    def _record(self, cs, fn, **kw):
        """``fn`` recorded into a new hipGraph on the capture stream and the trainer's graph pool (made on first use); ``kw``:
        torch.cuda.graph's (capture_error_mode).  Returns (graph, what fn returned)."""
        if self._graph_pool is None:
            self._graph_pool = torch.cuda.graph_pool_handle()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self._graph_pool, stream=cs, **kw):
            out = fn()
        return g, out

    def _bind_grads(self):
        """Every trainable parameter's .grad IS its view of the flat gradient buffer: autograd accumulates straight into the
        buffer the single all-reduce and the fused Adam read."""
        if not getattr(self, "_grads_bound", False):
            pd = dict(self.s.named_parameters())
            for n in self.flat.train_names:
                pd[n].grad = self.flat.grad_views[n]
            self._grads_bound = True

    def _dsmil_forward_backward(self, x, label, plan, teacher_feat, keep_num):
        """DSMIL student (scope row N1): kernel-backed autograd primitives (dsmil.py); loss, CE on the mixed logits and the
        per-class distillation with all three output gradients come from ONE head kernel."""
        from . import dsmil as DS
        from .mhim import _FeatureFn
        s = self.s
        self._bind_grads()
        if self.model_kind == "mhim":
            lb, li, B = s._dsmil_student(x, plan)
        else:
            lb, li, B, _ = s.online_encoder(_FeatureFn.apply(s, x, plan, s.feature[0].weight, s.feature[0].bias))
        Bt = teacher_feat[0].contiguous() if (teacher_feat is not None and self.aux_alpha != 0.) else None
        losses, g_lb, g_li, g_B = DS.dsmil_head(lb.detach(), li.detach(), label, B.detach().contiguous(), Bt, float(s.temp_t),
                                                self.main_alpha, self.aux_alpha, 1.0 / self.accum)
        self._backward_into_flat([lb, li, B], [g_lb, g_li, g_B])
        logits = 0.5 * (lb.detach() + li.detach())
        self._micro += 1
        self.last = {"logits": logits, "losses": losses, "patch_num": x.shape[0], "keep_num": keep_num, "exec": False}
        return logits, losses

    def _selfattn_forward_backward(self, x, label, plan, teacher_feat, keep_num, first):
        """TransMIL student: the encoder is a graph of kernel-backed autograd primitives (nystrom.py); every parameter's
        .grad IS its view of the flat gradient buffer, so autograd accumulates straight into the buffer the single
        all-reduce and the fused Adam read."""
        s, fl = self.s, self.flat
        gv = fl.grad_views
        self._bind_grads()
        if self.model_kind == "mhim":
            z = s._selfattn_student(x, plan)
        else:
            from .mhim import _FeatureFn
            z = s._encode(_FeatureFn.apply(s, x, plan, s.feature[0].weight, s.feature[0].bias))
        t_in = teacher_feat.view(-1) if (teacher_feat is not None and self.aux_alpha != 0.) else None
        # predictor + CE + distillation and their gradients in one kernel; accumulate: the buffer is zero after each update
        logits, losses, g_z, _, _ = ops.head_fwd_bwd(
            z.detach(), t_in, s.predictor.weight.data, s.predictor.bias.data, label, temp_t=float(s.temp_t),
            main_alpha=self.main_alpha, aux_alpha=self.aux_alpha, inv_accum=1.0 / self.accum,
            d_wp=gv["predictor.weight"], d_bp=gv["predictor.bias"], accumulate=True)
        self._backward_into_flat([z], [g_z])
        self._micro += 1
        self.last = {"logits": logits, "losses": losses, "patch_num": x.shape[0], "keep_num": keep_num, "exec": False}
        return logits, losses

    def _backward_into_flat(self, outs, g_outs):
        """torch.autograd.backward(outs, g_outs) with the parameter gradients landing in the flat buffer.  With .grad bound to the buffer's views autograd
        ADDS every parameter's gradient in a launch of its own (~30 launches of ~5 us, most of them for a few hundred floats, strung
        along the backward's chain); here .grad is empty during the backward - autograd just keeps the tensors our backward functions
        return - and ONE multi-tensor add moves them all into the buffer (which is zero after every update)."""
        fl = self.flat
        pd = getattr(self, "_train_params", None)
        if pd is None:
            named = dict(self.s.named_parameters())
            pd = self._train_params = [(named[n], fl.grad_views[n]) for n in fl.train_names]
        for p, _ in pd:
            p.grad = None
        torch.autograd.backward(outs, g_outs)
        views, grads = [], []
        for p, v in pd:
            if p.grad is not None:
                views.append(v)
                grads.append(p.grad.reshape(v.shape))
            p.grad = v
        if grads:
            torch._foreach_add_(views, grads)

    def _mid_hook(self):
        """Data parallel, eager steps: everything but the projection's gradient (the head of the flat buffer) is final - start its
        all-reduce (with the global-query tail) on RCCL's stream while mul_colsum + the dW1 GEMM + its slab reduction still run."""
        fl = self.flat
        fill_tail(fl.grad, fl.student, fl.n_train, self._chain)
        self._work_a = torch.distributed.all_reduce(fl.grad[self._split:], group=self.pg, async_op=True)

    def update(self):
        """All-reduce (data parallel) + fused Adam + EMA teacher.  Call once per ``accumulation_steps`` bags."""
        fl = self.flat
        if self._chain is not None and self._chain.tokens is None:
            raise mh.L.MhimxError("data-parallel update: this rank's step left no Merge tokens for the query chain (QueryChain) - the ranks "
                                  "would finish the update with different formulas for merge.global_q_mm")
        if self._work_a is not None:                       # overlapped form: the rest of the buffer, then wait for both halves
            work_b = torch.distributed.all_reduce(fl.grad[:self._split], group=self.pg, async_op=True)
            self._work_a.wait()
            work_b.wait()
            self._work_a = None
            scale = 1.0 / self.world
            finish_tail(fl.grad, fl.student, fl.n_train, scale, self._chain)
        else:
            scale = sync_flat_gradient(fl.grad, fl.student, fl.n_train, self.world, self.pg, self.comm, self._chain)
        self._apply(scale)

    def _all_reduce(self, buf):
        """The ONE collective of an update: SUM over the ranks (RCCL through torch.distributed, or the C-ABI's own handle)."""
        if self.comm is not None:
            self.comm.allreduce(buf)
        else:
            torch.distributed.all_reduce(buf, group=self.pg)

    def _apply(self, scale):
        fl = self.flat
        # the weights change below: this step's prepared weight images (ops.step_images, keyed by storage address) are stale from here
        # on, whoever runs the update - update(), or the captured data-parallel step (graph | all-reduce | graph), which never passes
        # through update() (an eval forward between replays picked up images of the pre-update weights)
        ops.step_images(None)
        fl.step += 1                                   # (the device-side counter was advanced by the step's prep launch)
        ops.optim_step(fl.student, fl.grad, fl.m, fl.v, fl.teacher if (self.model_kind == "mhim" and not fl.same_teacher) else None, fl.n_train,
                       fl.step, lr=self.lr, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.wd,
                       grad_scale=scale, ema_mm=self.mm, zero_grad=True, step_dev=self.opt_step, mm_table=self.mm_table,
                       lr_table=self.lr_table, g_extra=self._g_extra, clip_norm=self.clip_grad, ws=self._clip_ws, fold=self._fold_list)
        self._g_extra = None
        self._fold_list = None
        self._micro = 0

    def capture(self, bag, label, warmup=2, **kw):
        """Capture one whole train step on (bag, label) into a hipGraph and return it; ``graph.replay()`` then costs one
        launch instead of ~80.  The step must already have run eagerly (lazy one-time setup such as
        hipFuncSetAttribute cannot happen under capture), hence the warm-up calls."""
        assert self.accum == 1, "graph capture covers a full step (accumulation_steps == 1)"
        if self.s.mrh_sche is not None:
            # a captured graph freezes host-side schedule values: k, n_sel and len_keep are launch arguments and buffer shapes
            raise mh.L.MhimxError("capture(): the HAM-ratio schedule (mrh_sche) changes the number of masked rows per iteration; "
                                  "run such a model with eager train_step calls, or capture one graph per schedule value")
        # (a learning-rate schedule given as lr_sche and the EMA momentum schedule are device tables indexed by the device step counter:
        # they advance under replay; the scalar lr is a by-value kernel argument)
        self._capturing = True                             # (collectives stay outside the graphs: no mid-backward all-reduce)
        try:
            return self._capture(bag, label, warmup, **kw)
        finally:
            self._capturing = False

    def _capture(self, bag, label, warmup, **kw):
        # warm up ON the capture stream: autograd's gradient-accumulation nodes (TransMIL student) remember the stream they
        # were created on, and a node living on another stream would need a cross-stream event inside the capture
        step = lambda: self.train_step(bag, label, **kw)
        cs = self._capture_stream()
        self._warm_up(cs, step, warmup)
        torch.cuda.synchronize()
        if self.world > 1:
            # data parallel: the gradient all-reduce stays OUTSIDE the graphs (compute | RCCL all-reduce | optimiser): a
            # collective inside a captured graph depends on the RCCL build, and a rank that replays while another launches
            # eagerly would deadlock - two graph launches and one eager collective per step cost ~20 us of host time
            # The tail traffic around the collective (the non-trainable parameters / this rank's weighted Merge tokens into the buffer's
            # tail before the SUM, their average back into the student after it) is captured with the neighbouring graph: a replayed step
            # is graph | one collective | graph, nothing else on the host.  capture_error_mode "thread_local": the process group's
            # watchdog thread polls its events while we capture (a "global" capture would be invalidated by it).
            fl = self.flat
            def fb():
                self.forward_backward(bag, label, **kw)        # (leaves the QueryChain's tokens: static buffer of this capture)
                fill_tail(fl.grad, fl.student, fl.n_train, self._chain)
            g_fb, _ = self._record(cs, fb, capture_error_mode="thread_local")
            ops.step_images(None)                              # (graph-static images of the capture-time weights: never hand them out)
            self._all_reduce(fl.grad)
            scale = 1.0 / self.world
            def up():
                finish_tail(fl.grad, fl.student, fl.n_train, scale, self._chain)
                self._apply(scale)
            g_up, _ = self._record(cs, up, capture_error_mode="thread_local")
            fl.grad.zero_()                                # (the capture-time all-reduce summed stale values)
            return _SplitStep(self, g_fb, g_up)
        return self._record(cs, step)[0]

    def capture_steps(self, bags, labels, warmup=1, **kw):
        """ONE hipGraph of len(bags) consecutive COMPLETE train steps (each with its own update), bag after bag: a trainer that walks a
        resident dataset pays one graph launch per chunk of bags instead of one per bag (~6-8 us of launch latency between two replays of
        18-kernel graphs at c2: 2 % of a step).  One process, accumulation_steps == 1; the same step sequence as calling train_step on
        the bags in order (the dropout / draw streams advance through the device counters: replay-safe)."""
        assert self.accum == 1 and self.world == 1, "capture_steps: one process, one bag per update"
        if self.s.mrh_sche is not None:
            raise mh.L.MhimxError("capture_steps(): the HAM-ratio schedule changes the launch shapes per iteration")
        def steps():
            for b, l in zip(bags, labels):
                self.train_step(b, l, **kw)
        self._capturing = True
        try:
            cs = self._capture_stream()
            self._warm_up(cs, steps, warmup)
            torch.cuda.synchronize()
            return self._record(cs, steps)[0]
        finally:
            self._capturing = False

    def shape_cached(self, what, bag, label, i=None, cache=64):
        """``what`` = 'forward_backward' or 'train_step' on ``bag`` through a cache of captured hipGraphs keyed by the bag's SHAPE: the first
        bag of a shape runs eagerly (it is the kernels' warm-up), the second is captured - into buffers of the graph's own: the bag is copied
        into ONE buffer all the graphs share (they never run concurrently; so do they their memory pool), one launch - and replayed, every later
        one replays.  A dataset of bags of many sizes replays from its second epoch on.  The draw / dropout streams advance through the device
        step counter: replays draw fresh masks.  Only the single-pass ABMIL step is cached (``_nat_ok``: no host read-back, fixed launch
        shapes - a v1 mask ratio or a shape the one-pass kernels do not take runs eagerly), one process, cross entropy, accumulation_steps == 1.  The key
        holds everything a capture bakes in on the host: shape, the HAM-ratio schedule's row counts, the models' train / eval state, the
        Merge switch, the loss weights and - for 'train_step' - the optimiser's scalars.  ``cache``: the K most recently USED shapes stay.
        Returns (logits, losses, patch_num, keep_num) - the graph's static output buffers: read them before the next call - or None when
        the step cannot be cached (run it eagerly)."""
        x = bag[0] if bag.dim() == 3 else bag
        s, t = self.s, self.t
        if not (self.accum == 1 and self.world == 1 and self.loss == "ce" and x.is_cuda and x.dim() == 2 and not self._capturing and self._micro == 0):
            return None
        # the eager step's own route, asked of the bag as handed over ("exec" and "nat" are one answer here: a replay does not pay for telling
        # them apart).  mhimx_dsmil_mhim_window_run has no host read-back either; the teacher-free DSMIL call's shapes keep the form below
        r = self._step_route(x, label, i, None, None, executor=False)
        nat = r.name == "nat" or r.fam not in (None, _DSMIL)
        # (round 5) the TransMIL / DSMIL students: their step runs autograd over kernel-backed nodes whose gradient-accumulation nodes belong to
        # the stream they were first run on, so EVERY step of such a shape runs on the trainer's capture stream - eager on the first two
        # visits (the second is the capture's warm-up), captured on the third.  v2 recipe only (a v1 ratio reads a count back).
        auto = (not nat) and s.baseline in ("selfattn", "dsmil") and (self.model_kind != "mhim" or s.v2_counts(x.shape[0], i) is not None)
        if not (nat or auto):
            return None
        # (a HAM-ratio schedule, --mrh_sche, changes the row counts - the launch shapes - every few hundred iterations: they are part of the key)
        counts = s.v2_counts(x.shape[0], i) if self.model_kind == "mhim" else None
        st = self._shape_graphs
        if st is None:
            st = self._shape_graphs = {"graphs": {}, "seen": {}, "arena": None, "bad": set()}
        key = (what, tuple(x.shape), x.dtype, x.device.index, counts, s.training, None if t is None else t.training, s.merge_enable,
               float(self.main_alpha), float(self.aux_alpha), tuple(label.shape))
        # the optimiser's by-value scalars are baked into a captured update; scalars that come from a DEVICE table (lr_table / mm_table,
        # indexed by the device step counter) are not.  They are kept beside the graph, not in its key (with a host-side
        # scheduler every step had a new key, nothing was ever replayed and the visit counts grew without bound): a shape whose scalars
        # changed is captured again, and one whose scalars keep changing runs eagerly.
        scal = None
        if what == "train_step":
            scal = (None if self.lr_table is not None else float(self.lr), tuple(self.betas), float(self.eps), float(self.wd),
                    None if self.mm_table is not None else float(self.mm))
        if key in st["bad"]:
            return None
        ent = st["graphs"].get(key)
        if ent is not None and ent.scal != scal:
            st["graphs"].pop(key)
            ent = None
            n_re = st.setdefault("rescaled", {})
            n_re[key] = n_re.get(key, 0) + 1
            if n_re[key] > 2:
                st["bad"].add(key)
                st["seen"].pop(key, None)
                return None
            st["seen"][key] = 2                                  # (the shape is warm: capture on this visit)
        if len(st["seen"]) > 4096:                               # (visit counts of shapes that never came back)
            st["seen"] = {k_: v_ for k_, v_ in st["seen"].items() if k_ in st["graphs"]}
        fn = self.train_step if what == "train_step" else self.forward_backward
        if ent is None:
            st["seen"][key] = st["seen"].get(key, 0) + 1
            if st["seen"][key] < (3 if auto else 2):
                step = lambda: fn(bag, label, i=i)
                logits, losses = self._warm_up(self._capture_stream(), step) if auto else step()
                return logits, losses, self.last["patch_num"], self.last["keep_num"]
            while len(st["graphs"]) >= max(1, int(cache)):        # the least recently used shape makes room
                st["graphs"].pop(next(iter(st["graphs"])))
            need = x.numel()
            ar = st["arena"]
            if ar is None or ar.numel() < need or ar.dtype != x.dtype or ar.device != x.device:
                ar = st["arena"] = torch.empty(need, dtype=x.dtype, device=x.device)
            xs, ls = ar[:need].view(x.shape), torch.empty_like(label)
            cs = self._capture_stream()                           # (no warm-up here: the shape's earlier visits were it)
            torch.cuda.synchronize()
            micro, host_step = self._micro, self.flat.step

            def restore(failed):
                """The host's state as before the recording (a recording runs nothing); ``failed``: and nothing left pending."""
                self._micro, self.flat.step = micro, host_step
                if failed:
                    self._fold_list, self._defer = None, ops.ReduceList()
                ops.step_images(None)
            self._capturing = True
            try:
                g, (logits, losses) = self._record(cs, lambda: fn(xs, ls, i=i))      # (recorded, not run: the replay below is this bag's step)
            except Exception as exc:
                # a step that turned out not to be capturable (a host read-back somewhere): this shape runs eagerly from now on.  Argument
                # errors of the library (a label on the wrong device, a refused shape) are the caller's bug, not a capture problem: they
                # propagate; the first capture failure of every other kind is kept for inspection
                restore(True)
                if isinstance(exc, mh.L.MhimxError):
                    raise
                st["bad"].add(key)
                st.setdefault("errors", []).append(repr(exc))
                torch.cuda.synchronize()
                return None
            finally:
                self._capturing = False
            restore(False)
            ent = st["graphs"][key] = _ShapeGraph(g, xs, ls, logits, losses, self.last["patch_num"], self.last["keep_num"], dict(self.last), scal)
        else:
            st["graphs"][key] = st["graphs"].pop(key)             # most recently used: to the end of the (insertion-ordered) dict
        ent.x.copy_(x)
        ent.label.copy_(label)
        ent.graph.replay()
        if what == "train_step":
            self.flat.step += 1                                # (the host's count of updates: the device counter advanced in the graph)
            ops.step_images(None)
        else:
            self._micro += 1
        self.last = ent.last
        return ent.logits, ent.losses, ent.patch_num, ent.keep_num

    def train_step(self, bag, label, **kw):
        # (a step that is followed by its update right here may leave its last reductions to the update kernel: _nat_bag)
        self._fold_now = self.accum == 1 and self.world == 1 and not self.clip_grad
        try:
            out = self.forward_backward(bag, label, **kw)
        finally:
            self._fold_now = False
        if self._micro >= self.accum:
            self.update()
        return out
