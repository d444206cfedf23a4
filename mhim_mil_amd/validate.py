"""Validation path of the MHIM hot path.

``validate`` mirrors ``BaseTrainer.validate`` (engines/base_engine.py:234-329): every bag goes through the engine's
``validate_func`` (-> ``MHIM.forward_test`` on the HIP kernels), the logits stay on the device, the mean cross-entropy is
the reference's ``loss_cls_meter.avg``; ``get_metric_val`` mirrors engines/metrics.py:161-262 (same return tuples and
``rowd`` keys) with the torchmetrics collection replaced by one device evaluation (``ops.cls_metrics`` ->
mhimx_cls_metrics), including the DeterministicBootStrapper's resamples (engines/metrics.py:35-78): the resample indices
come from the same seeded ``torch.multinomial`` draw, so the sets are the reference's, and all resamples are evaluated in
the same four launches.

Survival datasets: ``surv_validate`` mirrors ``BaseTrainer.surv_validate`` (engines/base_engine.py:557-696) - the survival head of the
pass (hazards, survival curve, risk, NLL loss) is one launch over the logits (``ops.surv_nll`` -> mhimx_surv_nll), and
``get_surv_metrics`` / ``get_metric_val(surv=True)`` evaluate the censored concordance index of every bootstrap resample on the device
(``ops.cindex`` -> mhimx_cindex) where the reference makes ``num_bootstrap`` O(n^2) calls of sksurv on the host.
"""
from __future__ import annotations

from collections import OrderedDict

import torch

from . import ops

_BOOT_SEED = 7784414403328510413            # engines/metrics.py:154


def bootstrap_indices(n, num_bootstraps, seed, device):
    """The resamples the reference draws (engines/metrics.py:27-28,59-63): ONE generator seeded once, ``num_bootstraps``
    successive multinomial draws of n out of n with replacement."""
    g = torch.Generator()
    g.manual_seed(seed)
    w = torch.ones(n)
    idx = torch.stack([torch.multinomial(w, num_samples=n, replacement=True, generator=g) for _ in range(num_bootstraps)])
    return idx.to(device=device, dtype=torch.int64)


def get_cls_metrics(args, logits, labels, bootstrap, device=None):
    """engines/metrics.py:104-123.  Without bootstrap: seven python floats (Acc, AUC, Precision, Recall, F1, CK, Acc_micro);
    with: seven [mean, std] pairs in the reference's order."""
    C = int(args.n_classes)
    binm = C == 2 and bool(getattr(args, "bin_metric", False))
    logits = logits.detach().float().reshape(-1, C).contiguous()
    labels = labels.detach().reshape(-1).to(torch.int64).contiguous()
    if not bootstrap:
        m = ops.cls_metrics(logits, labels, C, binm)[0].cpu().tolist()
        return tuple(m)
    idx = bootstrap_indices(labels.numel(), int(args.num_bootstrap), int(getattr(args, "fold_curr", 0)) + _BOOT_SEED, logits.device)
    out = ops.cls_metrics(logits, labels, C, binm, sample_idx=idx).double()
    mean, std = out.mean(0).cpu().tolist(), (out.std(0) if out.shape[0] > 1 else torch.zeros(7)).cpu().tolist()
    return tuple([mean[i], std[i]] for i in range(7))


def get_surv_metrics(args, censorships, event_times, risk_scores, bootstrap=False):
    """engines/metrics.py:90-104.  ``censorships`` is what the reference passes under that name: the EVENT indicator
    (1 - censorship).bool() (engines/metrics.py:175).  Without bootstrap: the C-index as a python float; with: [mean, std] over the
    resamples of ``bootstrap_indices`` (mean and unbiased std in fp64 on the device; the reference rounds every resample's index to fp32
    first, engines/metrics.py:80 - here it is not).  A resample without a comparable pair raises, as sksurv does in the reference."""
    risk = risk_scores.detach().reshape(-1).float().contiguous()
    dev = risk.device
    event = (censorships.detach().reshape(-1) != 0).to(dev).contiguous()
    time = event_times.detach().reshape(-1).to(device=dev, dtype=torch.float64).contiguous()
    n = risk.numel()
    if not bootstrap:
        ci = float(ops.cindex(event, time, risk)[0, 0])
        if ci != ci:
            raise ops.L.MhimxError("get_surv_metrics: no comparable pair (the C-index is undefined)")
        return ci
    B = int(args.num_bootstrap)
    idx = bootstrap_indices(n, B, int(getattr(args, "fold_curr", 0)) + _BOOT_SEED, dev)
    per = max(1, min(ops.L.CINDEX_MAX_B, ops.L.CINDEX_MAX_BN // n))            # resamples one call takes
    ci = torch.cat([ops.cindex(event, time, risk, sample_idx=idx[lo:lo + per])[:, 0] for lo in range(0, B, per)])
    mean = ci.mean()
    std = ci.std() if B > 1 else torch.zeros((), dtype=torch.float64, device=dev)
    mean, std = torch.stack([mean, std]).cpu().tolist()
    if mean != mean:
        raise ops.L.MhimxError("get_surv_metrics: a bootstrap resample has no comparable pair (the C-index is undefined)")
    return [mean, std]


def _surv_metric_val(args, risk, bag_labels, model, status, early_stopping, epoch, loss_avg, suffix, boot):
    """The ``surv=True`` branch of engines/metrics.py:161-240."""
    cindex = get_surv_metrics(args, 1 - bag_labels["censorships"], bag_labels["event_times"], risk, bootstrap=boot)
    if boot and status == "val":
        cindex = cindex[0]
    if status == "val":
        stop = False
        if early_stopping is not None:
            early_stopping(args, epoch, -cindex, model)
            stop = early_stopping.early_stop
        rowd = OrderedDict((k + suffix, v) for k, v in (("cindex", cindex), ("loss", loss_avg)))
        return [cindex, cindex], stop, loss_avg, None, rowd
    if not boot:
        cindex = [cindex, 0]
    rowd = OrderedDict((k + suffix, v) for k, v in (("cindex", cindex[0]), ("cindex_std", cindex[1]), ("loss", loss_avg)))
    return [cindex[0], cindex[1]], loss_avg, rowd


def get_metric_val(args, bag_logit, bag_labels, model, status, early_stopping, epoch, loss_avg, suffix=None, surv=False):
    """engines/metrics.py:161-262.  ``surv=True``: ``bag_logit`` holds the risk scores and ``bag_labels`` is
    {'censorships', 'event_times'}; early stopping runs on -cindex."""
    boot = status in getattr(args, "bootstrap_mode", ())
    suffix = "" if suffix is None else "_" + str(suffix)
    if surv:
        return _surv_metric_val(args, bag_logit, bag_labels, model, status, early_stopping, epoch, loss_avg, suffix, boot)
    acc, auc, prec, rec, f1, ck, acc_micro = get_cls_metrics(args, bag_logit, bag_labels, boot)
    if boot and status == "val":
        acc, auc, prec, rec, f1, ck, acc_micro = acc[0], auc[0], prec[0], rec[0], f1[0], ck[0], acc_micro[0]
    if status == "val":
        stop = False
        if early_stopping is not None:
            early_stopping(args, epoch, -(auc if getattr(args, "best_metric_index", 0) == 0 else acc), model)
            stop = early_stopping.early_stop
        rowd = OrderedDict([("acc", acc), ("precision", prec), ("recall", rec), ("fscore", f1), ("auc", auc), ("ck", ck),
                            ("acc_micro", acc_micro), ("loss", loss_avg)])
        rowd = OrderedDict((k + suffix, v) for k, v in rowd.items())
        return [auc, acc, prec, rec, f1, ck, acc_micro], stop, loss_avg, None, rowd
    if not boot:
        acc, auc, prec, rec, f1, ck, acc_micro = ([v, 0] for v in (acc, auc, prec, rec, f1, ck, acc_micro))
    rowd = OrderedDict([("acc", acc[0]), ("precision", prec[0]), ("recall", rec[0]), ("fscore", f1[0]), ("auc", auc[0]),
                        ("ck", ck[0]), ("acc_micro", acc_micro[0]), ("loss", loss_avg), ("acc_std", acc[1]), ("fscore_std", f1[1]),
                        ("auc_std", auc[1]), ("ck_std", ck[1]), ("acc_micro_std", acc_micro[1])])
    rowd = OrderedDict((k + suffix, v) for k, v in rowd.items())
    return [auc[0], acc[0], prec[0], rec[0], f1[0], ck[0], acc_micro[0], auc[1], acc[1], f1[1], ck[1], acc_micro[1]], loss_avg, rowd


def _validate_chunked(engine, args, model, loader, criterion, chunk):
    """The loop of ``validate`` with ``chunk`` batches gathered per ``engine.validate_many`` call (MHIM.infer_many: one C call for bags
    of different sizes).  Same lists, same per-bag loss terms added in loader order."""
    logits_all, labels_all, loss_sum, count = [], [], None, 0

    def flush(bags, labels):
        nonlocal loss_sum, count
        lab = torch.cat(labels)
        logits, losses = engine.validate_many(args, model, bags, lab, criterion)
        for j in range(len(bags)):
            lg = logits[j:j + 1]
            logits_all.append(lg)
            labels_all.append(labels[j])
            loss = losses[j] if losses is not None else criterion(lg, labels[j])
            loss_sum = loss if loss_sum is None else loss_sum + loss
            count += 1

    bags, labels = [], []
    with torch.no_grad():
        for batch in loader:
            bag, label = batch["input"], batch["target"]
            dev = bag.device if bag.is_cuda else torch.device("cuda")
            bags.append(bag.to(dev, non_blocking=True))
            labels.append(label.to(dev, non_blocking=True).reshape(-1))
            if labels[-1].numel() != 1:
                raise ops.L.MhimxError("validate(chunk > 0): one bag and one label per batch (the reference's batch size 1)")
            if len(bags) == chunk:
                flush(bags, labels)
                bags, labels = [], []
        if bags:
            flush(bags, labels)
    return logits_all, labels_all, loss_sum, count


def validate(engine, args, model, loader, criterion=None, early_stopping=None, epoch=None, status="val", chunk=0):
    """engines/base_engine.py:234-329 for the MHIM models.  ``loader`` yields dicts with 'input' (bag [1,N,D] or [N,D]) and
    'target' ([1] int64) - the reference's batch layout (batch size 1).  Returns what BaseTrainer.validate returns.
    ``chunk`` > 0: that many batches are gathered and go through ``engine.validate_many`` together (mhimx_infer_run: one C call per
    chunk of bags of different sizes, the per-bag cross entropy computed on the device); 0: bag after bag through ``validate_func``."""
    model.eval()
    criterion = criterion or torch.nn.CrossEntropyLoss()
    if chunk > 0:
        logits_all, labels_all, loss_sum, count = _validate_chunked(engine, args, model, loader, criterion, int(chunk))
        bag_logit, bag_labels = torch.cat(logits_all), torch.cat(labels_all)
        loss_avg = float(loss_sum / count)
        return list(get_metric_val(args, bag_logit, bag_labels, model, status, early_stopping, epoch, loss_avg))
    logits_all, labels_all, loss_sum, count = [], [], None, 0
    with torch.no_grad():
        for i, batch in enumerate(loader):
            bag, label = batch["input"], batch["target"]
            dev = bag.device if bag.is_cuda else torch.device("cuda")
            bag, label = bag.to(dev, non_blocking=True), label.to(dev, non_blocking=True).reshape(-1)
            logits, labels = engine.validate_func(args, model=model, bag=bag, label=label, criterion=criterion, batch_size=label.numel(),
                                                  i=i, pos=batch.get("pos"))
            if logits is None:
                continue
            bs = logits.size(0)
            logits_all.append(logits.reshape(bs, -1))
            labels_all.append(label)
            loss = criterion(logits.view(bs, -1), labels.view(bs))
            loss_sum = loss if loss_sum is None else loss_sum + loss              # AverageMeter.update(loss, 1)
            count += 1
    bag_logit, bag_labels = torch.cat(logits_all), torch.cat(labels_all)
    loss_avg = float(loss_sum / count)
    return list(get_metric_val(args, bag_logit, bag_labels, model, status, early_stopping, epoch, loss_avg))


def surv_validate(engine, args, model, loader, criterion=None, early_stopping=None, epoch=None, status="val", chunk=0):
    """engines/base_engine.py:557-696 for the MHIM models.  ``loader`` yields dicts with 'input' (bag [1,N,D] or [N,D]), 'target' ([1]
    int64: the time bin), 'censorship' ([1]: 1 = censored) and 'event' ([1]: the event time) - the reference's batch layout (batch size 1);
    the model's ``n_classes`` is the number of time bins.  Returns what BaseTrainer.surv_validate returns.
    ``chunk`` > 0: that many batches are gathered, their logits come from ``engine.validate_many`` (for ABMIL and DSMIL the ragged
    inference calls) and the survival head runs once over the chunk; 0: bag after bag through ``validate_func``, the head once over the
    pass.  Either way the head is ``ops.surv_nll`` (hazards, survival curve, risk and the per-bag NLL loss of ``criterion.alpha`` in one
    launch), the loss is the mean of its per-bag losses, and the metric is computed from its risk scores without a trip to the host."""
    model.eval()
    alpha = float(getattr(criterion, "alpha", 0.0) or 0.0)
    chunk = int(chunk)
    risks, losses, cens, times = [], [], [], []
    bags, logits, Y, c = [], [], [], []

    def head():
        lg = engine.validate_many(args, model, bags, torch.cat(Y), None)[0] if chunk > 0 else torch.cat(logits)
        risk, loss = ops.surv_nll(lg.float(), torch.cat(Y), torch.cat(c), alpha=alpha)
        risks.append(risk)
        losses.append(loss)
        cens.extend(c)
        for lst in (bags, logits, Y, c):
            lst.clear()

    with torch.no_grad():
        for i, batch in enumerate(loader):
            bag = batch["input"]
            dev = bag.device if bag.is_cuda else torch.device("cuda")
            bag = bag.to(dev, non_blocking=True)
            label = batch["target"].to(device=dev, dtype=torch.int64, non_blocking=True).reshape(-1)
            cen = batch["censorship"].to(device=dev, dtype=torch.float32, non_blocking=True).reshape(-1)
            if chunk > 0:
                if label.numel() != 1:
                    raise ops.L.MhimxError("surv_validate(chunk > 0): one bag and one label per batch (the reference's batch size 1)")
                bags.append(bag)
            else:
                lg, _ = engine.validate_func(args, model=model, bag=bag, label=label, criterion=criterion, batch_size=label.numel(), i=i,
                                             pos=batch.get("pos"))
                if lg is None:
                    continue
                logits.append(lg.reshape(label.numel(), -1))
            Y.append(label)
            c.append(cen)
            times.append(batch["event"].to(dev, non_blocking=True).reshape(-1))
            if chunk > 0 and len(bags) == chunk:
                head()
        if Y:
            head()
    loss_avg = float(torch.cat(losses).mean())
    labels = {"censorships": torch.cat(cens), "event_times": torch.cat(times)}
    return list(get_metric_val(args, torch.cat(risks), labels, model, status, early_stopping, epoch, loss_avg, surv=True))
