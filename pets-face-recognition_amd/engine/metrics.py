"""Verification metrics of the evaluation epoch: what /root/reference/engine/controller.py:67-75,112-183 gets from torchmetrics
(ROC, AUROC, AveragePrecision, ConfusionMatrix, Accuracy / Precision / Recall(threshold=), StatScores(threshold=)) and the
index rules the reference applies itself (`Opt thr`, TAR@FAR / TH@FAR, TRR@FRR / TH@FRR), with no torchmetrics / sklearn
dependency.  Pinned to the reference's own `_evaluate` output: tests/golden/evaluate.npz.

Arithmetic follows the reference where it decides a discrete outcome: binary predictions are `score >= threshold` in the
scores' float32; fpr / tpr are integer counts divided in float32 (torchmetrics' `fps / fps[-1]`), so `argmin(fpr + 1 - tpr)`
(`Opt thr`, controller.py:120) and `argmin(fpr + fnr)` (`compute_accuracy`, 206-211) see the same ties.  The areas (AUROC, AP)
are accumulated in float64 — the reference prints their float32 values (tolerance 1e-6 in the tests).

The sort + running-count part runs on the device when the scores are CUDA tensors (`pfr_pair_curve`: one
workgroup bitonic-sorts the ≤ 20 000 pair scores with their labels and scans the genuine-pair count); every metric below is
a handful of operations on that one sorted list.  CPU tensors take the torch sort (BASELINE config 1)."""
import torch


class PairStats:
    """The pair scores of one validation set, sorted once (descending): `s` float32 scores, `y` 0/1 labels, both on the host."""

    def __init__(self, scores, labels):
        if scores.is_cuda:
            from .._hip import lib
            sc = scores.detach().float().contiguous().flatten()
            lb = labels.detach().to(sc.device).to(torch.int32).contiguous().flatten()
            P = sc.numel()
            st = torch.cuda.current_stream().cuda_stream
            ws = torch.empty(lib.pfr_pair_curve_ws_bytes(P), dtype=torch.uint8, device=sc.device)
            ss = torch.empty(P, dtype=torch.float32, device=sc.device)
            ct = torch.empty(P, dtype=torch.int32, device=sc.device)
            re = torch.empty(P, dtype=torch.uint8, device=sc.device)
            lib.pfr_pair_curve(sc.data_ptr(), lb.data_ptr(), P, ws.data_ptr(), ss.data_ptr(), ct.data_ptr(), re.data_ptr(), st)
            self.s = ss.cpu()
            self.tp_cum = ct.cpu().long()                       # genuine pairs among the first i+1 scores
            self.ends = torch.nonzero(re.cpu()).flatten()       # last position of every run of equal scores
            self.y = torch.diff(self.tp_cum, prepend=torch.zeros(1, dtype=torch.long))
        else:
            s = scores.detach().float().cpu().flatten()
            y = labels.detach().cpu().flatten().long()
            order = torch.argsort(s, descending=True, stable=True)
            self.s, self.y = s[order], y[order]
            self.tp_cum = torch.cumsum(self.y, 0)
            distinct = torch.nonzero(self.s[1:] != self.s[:-1]).flatten()
            self.ends = torch.cat([distinct, torch.tensor([self.s.numel() - 1])])
        self.n = self.s.numel()
        self.n_pos = int(self.tp_cum[-1]) if self.n else 0
        self.n_neg = self.n - self.n_pos

    # ---- curves: one operating point per distinct score (torchmetrics' _binary_clf_curve)
    def _counts(self):
        tps = self.tp_cum[self.ends]
        fps = 1 + self.ends - tps
        return tps, fps

    def roc(self):
        """→ fpr, tpr, thresholds (float32, descending thresholds, first point (0, 0) at max + 1: torchmetrics.ROC)"""
        tps, fps = self._counts()
        z = torch.zeros(1, dtype=torch.long)
        tps, fps = torch.cat([z, tps]), torch.cat([z, fps])
        thr = torch.cat([self.s[self.ends][:1] + 1, self.s[self.ends]])
        # (a set without impostor / without genuine pairs: rates 0 instead of torchmetrics' 0/0 = nan)
        return fps / fps[-1].clamp_min(1), tps / tps[-1].clamp_min(1), thr

    def auroc(self):
        tps, fps = self._counts()
        z = torch.zeros(1, dtype=torch.double)
        tpr = torch.cat([z, tps.double() / max(self.n_pos, 1)])
        fpr = torch.cat([z, fps.double() / max(self.n_neg, 1)])
        return float(torch.trapz(tpr, fpr))

    def average_precision(self):
        """AP = Σ (R_n − R_{n−1})·P_n over the distinct score thresholds (ties share one operating point)"""
        tps, fps = self._counts()
        prec = tps.double() / (tps + fps).double()
        rec = tps.double() / max(self.n_pos, 1)
        prev = torch.cat([torch.zeros(1, dtype=torch.double), rec[:-1]])
        return float(((rec - prev) * prec).sum())

    def opt_threshold(self):
        """`thresholds[argmin(fpr + 1 - tpr)]` (controller.py:120), float32 arithmetic in the reference's operand order"""
        fpr, tpr, thr = self.roc()
        return float(thr[torch.argmin(fpr + 1 - tpr)])

    # ---- counts at a threshold: prediction = score >= thr in float32 (torchmetrics' binary input handling)
    def stats_at(self, thr):
        t = torch.as_tensor(thr).to(torch.float32)
        npred = int((self.s >= t).sum())            # s is descending: the predicted-positive scores are a prefix
        tp = int(self.tp_cum[npred - 1]) if npred else 0
        fp = npred - tp
        fn = self.n_pos - tp
        tn = self.n_neg - fp
        return dict(tp=tp, fp=fp, tn=tn, fn=fn,
                    accuracy=(tp + tn) / max(1, self.n),
                    precision=tp / (tp + fp) if tp + fp else 0.0,     # torchmetrics: zero_division = 0
                    recall=tp / (tp + fn) if tp + fn else 0.0)

    def best_threshold_accuracy(self, thresholds=None, fpr=None, fnr=None):
        """accuracy at t = thresholds[argmin(fpr + fnr)] with `score > t` as the decision (Controller.compute_accuracy,
        controller.py:206-211) → (accuracy, t)"""
        if thresholds is None:
            fpr, tpr, thresholds = self.roc()
            fnr = 1 - tpr
        t = thresholds[torch.argmin(fpr + fnr)].to(torch.float32)
        gt = self.s > t
        n_true = int((gt & (self.y == 1)).sum()) + int((~gt & (self.y == 0)).sum())
        return n_true / max(1, self.n), float(t)

    # ---- the reference's own index rules (controller.py:162-181)
    def far_points(self, far_thrs):
        """for every far: thr = neg_scores[-int(len(neg) * far)] on the ascending impostor scores (index −0 is index 0, as in the
        reference); skipped when thr is exactly 0 or 1; TAR = #(genuine >= thr) / #genuine → {far: (tar, thr)}"""
        neg = self.s[self.y == 0].flip(0)
        out = {}
        for far in far_thrs:
            thr = neg[-int(len(neg) * far)]
            if float(thr) not in (0.0, 1.0):
                out[far] = (self.stats_at(thr)['tp'] / self.n_pos, float(thr))
        return out

    def frr_points(self, frr_thrs):
        """thr = pos_scores[int(len(pos) * frr)] on the ascending genuine scores; TRR = #(impostor < thr) / #impostor"""
        pos = self.s[self.y == 1].flip(0)
        out = {}
        for frr in frr_thrs:
            thr = pos[int(len(pos) * frr)]
            if float(thr) not in (0.0, 1.0):
                out[frr] = (self.stats_at(thr)['tn'] / self.n_neg, float(thr))
        return out


class HistStats:
    """Verification metrics from the genuine / impostor score HISTOGRAMS of every pair (match.pair_histogram): `hist` int64
    [2, bins + 1] (row 1 = genuine, last slot = NaN scores), with the bin of a score s = clamp(floor((s - lo) * inv_w), 0, bins - 1).
    Operating point b (0 .. bins): a pair is predicted positive when its bin is >= b, so TP(b) / FP(b) are suffix sums of the two
    rows (b = bins predicts nothing).  The NaN slot is reported as `n_nan` and takes part in no rate.  Thresholds are the lower
    edge lo + b / inv_w of bin b, mapped to the reference's similarity (cos + 1) / 2 when `to_similarity`."""

    def __init__(self, hist, lo, inv_w, to_similarity=True):
        h = torch.as_tensor(hist).detach().cpu().long()
        if h.dim() != 2 or h.shape[0] != 2 or h.shape[1] < 2:
            raise ValueError("HistStats: hist must be [2, bins + 1]")
        self.bins = h.shape[1] - 1
        self.lo, self.inv_w, self.to_similarity = float(lo), float(inv_w), bool(to_similarity)
        self.neg, self.pos = h[0, :self.bins], h[1, :self.bins]
        self.n_nan = int(h[:, self.bins].sum())
        self.n_pos, self.n_neg = int(self.pos.sum()), int(self.neg.sum())
        z = torch.zeros(1, dtype=torch.long)
        # suffix sums, index b = 0 .. bins
        self.tp = torch.cat([self.pos.flip(0).cumsum(0).flip(0), z])
        self.fp = torch.cat([self.neg.flip(0).cumsum(0).flip(0), z])

    def threshold(self, b):
        t = self.lo + b / self.inv_w
        return (t + 1) / 2 if self.to_similarity else t

    def auroc(self):
        """trapezoid over the operating points in float64: the pairs inside one bin count as ties (half a win each)"""
        tpr = self.tp.double().flip(0) / max(self.n_pos, 1)
        fpr = self.fp.double().flip(0) / max(self.n_neg, 1)
        return float(torch.trapz(tpr, fpr))

    def eer(self):
        """equal error rate: (FAR + FRR) / 2 at the operating point where |FAR - FRR| is smallest (ties: the lowest bin)"""
        far = self.fp.double() / max(self.n_neg, 1)
        frr = 1 - self.tp.double() / max(self.n_pos, 1)
        b = int(torch.argmin((far - frr).abs()))
        return float((far[b] + frr[b]) / 2)

    def stats_at_bin(self, b):
        b = int(b)
        if not 0 <= b <= self.bins:
            raise ValueError(f"HistStats: operating point {b} outside 0..{self.bins}")
        tp, fp = int(self.tp[b]), int(self.fp[b])
        fn, tn = self.n_pos - tp, self.n_neg - fp
        return dict(tp=tp, fp=fp, tn=tn, fn=fn, threshold=self.threshold(b),
                    tar=tp / self.n_pos if self.n_pos else 0.0, far=fp / self.n_neg if self.n_neg else 0.0,
                    accuracy=(tp + tn) / max(1, self.n_pos + self.n_neg))

    def far_points(self, fars):
        """for every far: the smallest b with FP(b) / n_neg <= far — the most permissive threshold that does not exceed it (b = bins,
        which accepts nothing, always qualifies; the comparison is on integers: FP(b) <= far * n_neg evaluated as FP(b) / n_neg <= far
        in float64) → {far: (TAR, threshold, achieved FAR)}"""
        out = {}
        rate = self.fp.double() / max(self.n_neg, 1)          # non-increasing in b
        for far in fars:
            ok = torch.nonzero(rate <= float(far)).flatten()
            b = int(ok[0])
            st = self.stats_at_bin(b)
            out[far] = (st['tar'], st['threshold'], st['far'])
        return out


class RankStats:
    """Retrieval metrics from the exact ranks of every query's positives (match.positive_ranks): `ranks` int [Nq, Pmax], 1-based,
    ascending per row, 0 padded; `npos` int [Nq].  A query is valid when it has a positive.  With r_(1) < … < r_(n) the ranks of a valid
    query:  AP = (1 / n) Σ_k k / r_(k);  INP = n / r_(n);  first = r_(1).  Everything is summed in float64 on the host."""

    def __init__(self, ranks, npos):
        r = torch.as_tensor(ranks).detach().cpu().long()
        n = torch.as_tensor(npos).detach().cpu().long().reshape(-1)
        if r.dim() != 2 or r.shape[0] != n.numel():
            raise ValueError("RankStats: ranks [Nq, Pmax] with npos [Nq]")
        if n.numel() and (int(n.max()) > r.shape[1] or int(n.min()) < 0):
            raise ValueError("RankStats: npos outside 0..Pmax")
        valid = n > 0
        r, n = r[valid], n[valid]
        self.queries = int(n.numel())
        k = torch.arange(1, r.shape[1] + 1)
        used = k[None, :] <= n[:, None]
        if bool((used & (r < 1)).any()):
            raise ValueError("RankStats: a rank below 1 among the first npos entries of a row")
        nd = n.double()
        self.ap = (torch.where(used, k[None, :].double() / r.clamp_min(1).double(), torch.zeros((), dtype=torch.float64))).sum(dim=1) / nd
        last = torch.gather(r, 1, (n - 1)[:, None]).reshape(-1) if self.queries else n
        self.inp = nd / last.double()
        self.first = r[:, 0] if r.shape[1] else n

    def _mean(self, x):
        return float(x.double().mean()) if self.queries else float('nan')

    def mean_ap(self):
        return self._mean(self.ap)

    def mean_inp(self):
        return self._mean(self.inp)

    def cmc(self, k):
        """share of the valid queries whose best positive is among the first k"""
        return self._mean(self.first <= int(k))

    def mean_first_rank(self):
        return self._mean(self.first)

    def metrics(self, ks=(1, 5, 10)):
        out = {'mAP': self.mean_ap(), 'mINP': self.mean_inp()}
        out.update((f'CMC@K={int(k)}', self.cmc(k)) for k in ks)
        out['mean_first_rank'] = self.mean_first_rank()
        out['queries'] = self.queries
        return out


class ClusterStats:
    """Clustering metrics against class labels: `labels` int [N] (cluster of every item, e.g. match.cluster), `classes` int [N].  Built
    from the contingency counts n_kc (items of cluster k with class c) of the N (cluster, class) pairs — torch.unique, exact int64
    arithmetic, nothing cluster x class is built.  With a_k = Σ_c n_kc (cluster sizes) and b_c = Σ_k n_kc (class sizes):
      pairwise  TP = Σ n_kc (n_kc - 1) / 2;  precision = TP / Σ a_k (a_k - 1) / 2;  recall = TP / Σ b_c (b_c - 1) / 2
      BCubed    precision = (1 / N) Σ n_kc² / a_k;  recall = (1 / N) Σ n_kc² / b_c       (float64 sums on the host)
      F = 2 P R / (P + R).  A ratio with a zero denominator is NaN ("nothing to measure").
    `noise` (e.g. -1 for match.dbscan): the items with that label belong to no cluster — each is scored as a cluster of ONE (no predicted
    pair, BCubed precision 1), not all of them as one big cluster; `self.noise` is their count, `clusters` and `singletons` leave them
    out, and metrics() appends a 'noise' key.  noise=None: nothing changes."""

    def __init__(self, labels, classes, noise=None):
        k = torch.as_tensor(labels).detach().cpu().long().reshape(-1)
        c = torch.as_tensor(classes).detach().cpu().long().reshape(-1)
        if k.numel() != c.numel():
            raise ValueError("ClusterStats: labels [N] with classes [N]")
        self.n = int(k.numel())
        self.noise = None
        if noise is not None:
            is_noise = k == int(noise)
            self.noise = int(is_noise.sum())
            if self.noise:      # every noise item gets a label of its own: ranks after the clusters' (torch.unique below sees ranks only)
                k = torch.unique(k, return_inverse=True)[1]
                k[is_noise] = self.n + torch.arange(self.noise)
        uk, ik, a = torch.unique(k, return_inverse=True, return_counts=True)
        uc, ic, b = torch.unique(c, return_inverse=True, return_counts=True)
        # one int64 key per item: (cluster rank, class rank)
        key, n = torch.unique(ik * max(int(uc.numel()), 1) + ic, return_counts=True)
        ak, bc = a[key // max(int(uc.numel()), 1)], b[key % max(int(uc.numel()), 1)]
        pairs = lambda x: int((x * (x - 1) // 2).sum())
        self.tp, self.cluster_pairs, self.class_pairs = pairs(n), pairs(a), pairs(b)
        self.clusters = int(uk.numel()) - (self.noise or 0)
        self.singletons = int((a == 1).sum()) - (self.noise or 0)
        n2 = n.double() * n.double()
        self._b3p = float((n2 / ak.double()).sum()) / self.n if self.n else float('nan')
        self._b3r = float((n2 / bc.double()).sum()) / self.n if self.n else float('nan')

    @staticmethod
    def _ratio(x, y):
        return x / y if y else float('nan')

    @staticmethod
    def _f(p, r):
        return 2.0 * p * r / (p + r) if p + r > 0 else float('nan')      # (a NaN operand fails the compare)

    def pairwise(self):
        """(precision, recall, F)"""
        p, r = self._ratio(self.tp, self.cluster_pairs), self._ratio(self.tp, self.class_pairs)
        return p, r, self._f(p, r)

    def bcubed(self):
        """(precision, recall, F)"""
        return self._b3p, self._b3r, self._f(self._b3p, self._b3r)

    def metrics(self):
        p, r, f = self.pairwise()
        bp, br, bf = self.bcubed()
        out = {'pairwise_precision': p, 'pairwise_recall': r, 'pairwise_f': f, 'bcubed_precision': bp, 'bcubed_recall': br,
               'bcubed_f': bf, 'clusters': self.clusters, 'singletons': self.singletons}
        if self.noise is not None:
            out['noise'] = self.noise
        return out


class OpenSetStats:
    """Open-set identification (NIST 1:N: FNIR@FPIR; also DIR@FAR) from the per-probe extremes of match.class_extremes: `pos_score`,
    `pos_index` the best mate (index -1: the probe has no mate), `neg_score`, `neg_index` the best impostor (index -1: none).  Every probe
    is searched against all the others, leave-one-out.  The rank order is (score descending, index ascending).
      MATED probes M = {x : pos_index[x] >= 0}; x is a HIT iff its best mate ranks before its best impostor, or it has no impostor.
      NON-MATED searches: every probe with an impostor, searched against the gallery WITHOUT its own class: its top score is neg_score[x];
        n = their number;  fpir(t) = #{neg_score >= t} / n.
      threshold_at_fpir(f) = the smallest float32 t with #{neg_score >= t} <= floor(f n): nextafter above the (floor(f n) + 1)-th largest
        impostor score, -inf when floor(f n) >= n.  (f n is taken exactly, from the decimal digits of f: 0.29 * 100 is 29.)
      dir_at_fpir(f) = #{x in M : hit and pos_score[x] >= threshold_at_fpir(f)} / |M|;  fnir_at_fpir = 1 - dir_at_fpir.
    A ratio with a zero denominator is NaN."""

    def __init__(self, pos_score, pos_index, neg_score, neg_index):
        f32 = lambda t: torch.as_tensor(t).detach().cpu().float().reshape(-1)
        i64 = lambda t: torch.as_tensor(t).detach().cpu().long().reshape(-1)
        ps, pi, ns, ni = f32(pos_score), i64(pos_index), f32(neg_score), i64(neg_index)
        if not ps.numel() == pi.numel() == ns.numel() == ni.numel():
            raise ValueError("OpenSetStats: four vectors of one length")
        self.mated = pi >= 0
        has_neg = ni >= 0
        before = (ps > ns) | ((ps == ns) & (pi < ni))
        self.hit = self.mated & (~has_neg | before)
        self.pos_score = ps
        self.n_mated = int(self.mated.sum())
        self.neg_sorted = ns[has_neg].sort(descending=True).values
        self.n = int(self.neg_sorted.numel())

    def rank1(self):
        return int(self.hit.sum()) / self.n_mated if self.n_mated else float('nan')

    def fpir(self, t):
        return int((self.neg_sorted >= float(t)).sum()) / self.n if self.n else float('nan')

    def threshold_at_fpir(self, f):
        from fractions import Fraction
        k = int(Fraction(repr(float(f))) * self.n // 1)
        if k >= self.n:
            return float('-inf')
        return float(torch.nextafter(self.neg_sorted[max(k, 0)], torch.tensor(float('inf'))))

    def dir_at_fpir(self, f):
        if not self.n_mated:
            return float('nan')
        return int((self.hit & (self.pos_score >= self.threshold_at_fpir(f))).sum()) / self.n_mated

    def fnir_at_fpir(self, f):
        return 1.0 - self.dir_at_fpir(f)

    def metrics(self, fpirs=(0.1, 0.01)):
        out = {'rank1': self.rank1()}
        for f in fpirs:
            out[f'DIR@FPIR={f}'] = self.dir_at_fpir(f)
            out[f'TH@FPIR={f}'] = self.threshold_at_fpir(f)
        return out


# ---- function forms (one sort per call)
def roc_curve(scores, labels):
    return PairStats(scores, labels).roc()


def auroc(scores, labels):
    return PairStats(scores, labels).auroc()


def average_precision(scores, labels):
    return PairStats(scores, labels).average_precision()


def best_threshold_accuracy(scores, labels, thresholds, fpr, fnr):
    return PairStats(scores, labels).best_threshold_accuracy(thresholds, fpr, fnr)


def stats_at_threshold(scores, labels, thr):
    return PairStats(scores, labels).stats_at(thr)


def rank_metrics(ranks, npos, ks=(1, 5, 10)):
    return RankStats(ranks, npos).metrics(ks)


def cluster_metrics(labels, classes):
    return ClusterStats(labels, classes).metrics()
