"""`Controller` — the model + loss + evaluation unit, with the method names of the reference's LightningModule
(/root/reference/engine/controller.py:14-246) but no PyTorch-Lightning dependency:

  Controller(config)                      model_loss = config.loss(config, config.model())        (17-22)
  training_step(batch, idx) -> loss       model_loss(batch['x'], batch['label'])['loss']           (27-29)
  validation_step / test_step -> dict     {'emb', 'label', 'index'}                                (31-35, 42-46)
  validation_epoch_end / test_epoch_end   outputs is List[dataloader][batch] (engine/loops/eval_loop.py:30-51)
  _evaluate, compute_accuracy, *_dataloader, configure_optimizers                                   (95-246)

The O(N²) python pair loop of the reference (77-90, 143-160: ≈ 8.4 µs per scored pair) is replaced by the match module
(one MFMA GEMM per gallery chunk + running top-K); the metrics dict has the reference's keys and threshold rules (pinned to the
reference's own `_evaluate` run, tests/golden/evaluate.npz).
Unlike the reference (39: `self.logger.run_id` unconditionally), a missing logger is fine."""
import json
import time
from pathlib import Path

import torch
import torch.nn as nn

from . import metrics as M
from ..match import recall_at_k, pair_similarity, pair_histogram, positive_ranks, cluster, dbscan, class_extremes, label_suspects


class Controller(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        model = self.config.model()
        self.model_loss = self.config.loss(config, model)
        self.hparams = {k: repr(v) for k, v in config.items()}
        self.logger = None
        self.current_epoch = 0
        self.last_metrics = {}
        self.align_rejected = 0          # frames the landmark alignment rejected so far (config.device_align)
        self.last_align_valid = None

    def forward(self, *args, **kwargs):
        return self.model_loss(*args, **kwargs)

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, config=None, map_location='cpu', strict=True, **_):
        """`Controller.load_from_checkpoint(path, config=get_dict_wrapper(cfg.py))` — how the reference's inference consumers get
        their FE models (generate_tsv.py:158-176, eval_fe_*.py).  Reads this package's checkpoints (a plain state dict with the
        reference's key names) and pytorch-lightning ones ({'state_dict': …}); the result is in eval()-ready train mode like PL's."""
        if config is None:
            raise ValueError("load_from_checkpoint needs config=… (the module is rebuilt from config.model() / config.loss())")
        ckpt = torch.load(str(checkpoint_path), map_location=map_location)
        sd = ckpt.get('state_dict', ckpt) if isinstance(ckpt, dict) else ckpt
        self = cls(config)
        self.load_state_dict(sd, strict=strict)
        return self

    # ------------------------------------------------------------------ steps
    def _images(self, x, train):
        """uint8 [N, H, W, 3] batches are raw frames: the config's device-side Compose pipeline (the reference's
        train_augmentation / val_augmentation, fe_dogs_config.py:17-32) turns them into the float NCHW batch.  A dict with 'data'
        and 'shape' is a ragged batch of raw frames (data_loading/ragged.py) and goes through the same config entries, whose fit
        stage brings it to the network's canvas first.
        `x` may be the whole batch dict: when the config defines `device_align` (data_loading/align.py; `device_train_align`, if
        defined, in training) and the batch carries the landmarks 'pts' (and optionally 'mask'), a ragged batch['x'] is aligned first
        (the reference's preprocessor/align.py) and the uniform uint8 result continues like any uniform uint8 batch.  The frames
        the solve rejected are counted in `align_rejected`; `last_align_valid` holds the flags of this batch (None: not aligned)."""
        self.last_align_valid = None
        if isinstance(x, dict) and 'x' in x:
            batch, x = x, x['x']
            align = self.config.get('device_align')
            if train and self.config.get('device_train_align') is not None:
                align = self.config.get('device_train_align')
            if align is not None and 'pts' in batch and isinstance(x, dict) and 'data' in x and 'shape' in x:
                x, valid = align(x, batch['pts_host'] if 'pts_host' in batch else batch['pts'], batch.get('mask'))
                self.last_align_valid = valid
                self.align_rejected += int((~valid).sum())
        if isinstance(x, dict) and 'data' in x and 'shape' in x:
            aug = self.config.get('device_train_augmentation' if train else 'device_val_augmentation')
            if aug is None:
                raise ValueError("ragged image batch but the config defines no device_train_augmentation / device_val_augmentation")
            return aug(x)
        if x.dtype != torch.uint8:
            return x
        aug = self.config.get('device_train_augmentation' if train else 'device_val_augmentation')
        if aug is None:
            raise ValueError("uint8 image batch but the config defines no device_train_augmentation / device_val_augmentation")
        return aug(x)

    def training_step(self, batch, batch_idx=0):
        x, label = self._images(batch, True), batch['label']
        if self.last_align_valid is not None and not self.last_align_valid.all():
            # frames whose landmarks the solve rejected come back all zero: they are DROPPED from the step, never trained on
            keep = torch.from_numpy(self.last_align_valid).to(label.device)
            if not bool(self.last_align_valid.any()):
                raise ValueError("training_step: the alignment rejected every frame of the batch")
            x, label = x[keep], label[keep]
        out = self.model_loss(x, label)
        # a MagFace head's length regulariser (part of the loss already): kept for the Trainer's loss line
        self.last_regulariser = out.get('loss_g') if isinstance(out, dict) else None
        # the pair term on the batch's Gram matrix (losses/pair.py; part of the loss already, with its weight): likewise
        self.last_pair_loss = out.get('loss_pair') if isinstance(out, dict) else None
        return out['loss']

    def validation_step(self, batch, batch_idx=0, dataset_idx=0):
        out = {'emb': self.model_loss(self._images(batch, False)), 'label': batch['label'], 'index': batch['index']}
        if self.last_align_valid is not None:
            # evaluation keeps every row (the pair lists index the set by position); the rejected frames are reported, 'Align rejected'
            out['align_rejected'] = int((~self.last_align_valid).sum())
        return out

    def test_step(self, batch, batch_idx=0, dataset_idx=0):
        return self.validation_step(batch, batch_idx, dataset_idx)

    @staticmethod
    def _align_rejected(outputs_i):
        """{'Align rejected': n} when the set went through device_align, {} otherwise"""
        if not any('align_rejected' in o for o in outputs_i):
            return {}
        return {'Align rejected': sum(o.get('align_rejected', 0) for o in outputs_i)}

    # ------------------------------------------------------------------ evaluation
    @staticmethod
    def _gather(outputs_i):
        emb = torch.cat([o['emb'] for o in outputs_i], dim=0)
        classes = torch.cat([o['label'] for o in outputs_i], dim=0)
        indices = torch.cat([o['index'] for o in outputs_i], dim=0)
        order = torch.argsort(indices)
        return emb[order].float(), classes[order]

    def _pair_scores(self, emb, pair_generator):
        ci = pair_generator.corrected_indices
        ia = [a for a, _ in ci]
        ib = [b for _, b in ci]
        sim = getattr(self.config, 'similarity_f', None)
        if sim is not None and not getattr(sim, '_is_default_cosine', False):
            # a custom similarity is always honoured (the reference calls config.similarity_f unconditionally,
            # controller.py:62) — on CUDA embeddings too; only the flagged default (cos+1)/2 takes the fused kernel
            scores = sim([(emb[a], emb[b]) for a, b in ci])
        else:
            scores = pair_similarity(emb, ia, ib)                       # (cos + 1) / 2, fe_dogs_config.py:89-93
        # CUDA scores stay on the device: the sort / scan of the metric suite runs there (engine/metrics.py, pfr_pair_curve)
        return scores.float(), torch.as_tensor(pair_generator.labels)

    def _recall(self, emb, classes, ks):
        dt = torch.float32 if not emb.is_cuda else getattr(self.config, 'match_dtype', torch.bfloat16)
        return recall_at_k(emb, classes, tuple(ks), compute_dtype=dt)

    def _rerank_recall(self, emb, classes, ks):
        """Opt-in (config.rerank = dict(k1=…, k2=…, lambda_value=…[, candidates=…])): Recall@K of the k-reciprocal re-ranked order
        (match.rerank) next to the cosine-order Recall@K, as 'Rerank Recall@K={k}'."""
        rr = self.config.get('rerank')
        if rr is None or not len(ks):
            return {}
        dt = torch.float32 if not emb.is_cuda else getattr(self.config, 'match_dtype', torch.bfloat16)
        rk = recall_at_k(emb, classes, tuple(ks), compute_dtype=dt, rerank=dict(rr))
        return {f'Rerank Recall@K={k}': (x / y if y else float('nan')) for k, (x, y) in rk.items()}

    def _retrieval(self, emb, classes):
        """Opt-in (config.retrieval = dict(ks=[1, 5, 10])): the re-ID retrieval metrics from the exact rank of every positive of every
        query among all the other items (match.positive_ranks: the match GEMM with a rank-counting epilogue on the device) — 'mAP',
        'mINP', 'CMC@K={k}' over ks, 'Mean first rank'.  NaN when no item has a same-class other."""
        rt = self.config.get('retrieval')
        if rt is None:
            return {}
        ks = [int(k) for k in dict(rt).get('ks', (1, 5, 10))]
        dt = torch.float32 if not emb.is_cuda else getattr(self.config, 'match_dtype', torch.bfloat16)
        m = M.RankStats(*positive_ranks(emb, classes, compute_dtype=dt)).metrics(ks)
        out = {'mAP': m['mAP'], 'mINP': m['mINP']}
        out.update((f'CMC@K={k}', m[f'CMC@K={k}']) for k in ks)
        out['Mean first rank'] = m['mean_first_rank']
        return out

    def _all_pairs(self, emb, classes):
        """Opt-in (config.all_pairs_far, a list of FARs): verification metrics over EVERY pair of the validation set from the genuine /
        impostor score histograms (match.pair_histogram: one GEMM with a histogram epilogue on the device) instead of the sampled pair
        list — TAR at FAR 1e-4 .. 1e-6 needs the ~N^2 / 2 impostor pairs.  Thresholds are similarities (cos + 1) / 2 like TH@FAR."""
        fars = self.config.get('all_pairs_far')
        if fars is None:
            return {}
        dt = torch.float32 if not emb.is_cuda else getattr(self.config, 'match_dtype', torch.bfloat16)
        hist, lo, inv_w = pair_histogram(emb, classes, bins=int(self.config.get('all_pairs_bins', 4096)), compute_dtype=dt)
        hs = M.HistStats(hist, lo, inv_w)
        out = {'AllPairs ROC AUC': hs.auroc(), 'AllPairs EER': hs.eer()}
        pts = hs.far_points(list(fars))
        out.update((f'AllPairs TAR@FAR={far}', pts[far][0]) for far in fars)
        out.update((f'AllPairs TH@FAR={far}', pts[far][1]) for far in fars)
        return out

    def _cluster(self, emb, classes, ps):
        """Opt-in (config.cluster = dict(thresholds=[0.8, 'opt', …])): identity clustering of the set at each threshold — single linkage,
        the connected components of the pairs at or above it (match.cluster: the match GEMM with a union-find epilogue on the device) —
        scored against the classes (engine.metrics.ClusterStats): pairwise F / precision / recall, BCubed F and the number of clusters.
        Thresholds are similarities (cos + 1) / 2 like 'Opt thr' and TH@FAR; the string 'opt' is this run's PairStats.opt_threshold().
        The kernels compare the cosine with float32(2 t - 1): that one rounding is the only difference to comparing similarities."""
        cl = self.config.get('cluster')
        if cl is None:
            return {}
        thrs = list(dict(cl).get('thresholds', ()))
        dt = torch.float32 if not emb.is_cuda else getattr(self.config, 'match_dtype', torch.bfloat16)
        stats = []
        for t in thrs:
            sim = float(ps.opt_threshold()) if isinstance(t, str) and t == 'opt' else float(t)
            stats.append(M.ClusterStats(cluster(emb, 2.0 * sim - 1.0, compute_dtype=dt), classes))
        out = {}
        out.update((f'Cluster F thr={t}', st.pairwise()[2]) for t, st in zip(thrs, stats))
        out.update((f'Cluster precision thr={t}', st.pairwise()[0]) for t, st in zip(thrs, stats))
        out.update((f'Cluster recall thr={t}', st.pairwise()[1]) for t, st in zip(thrs, stats))
        out.update((f'Cluster BCubed F thr={t}', st.bcubed()[2]) for t, st in zip(thrs, stats))
        out.update((f'Clusters thr={t}', st.clusters) for t, st in zip(thrs, stats))
        return out

    def _dbscan(self, emb, classes, ps):
        """Opt-in (config.dbscan = dict(thresholds=[0.8, 'opt', …], min_samples=4)): DBSCAN identity clustering of the set at each
        threshold (match.dbscan: two passes of the match GEMM on the device), scored against the classes with every noise item as a
        cluster of its own (engine.metrics.ClusterStats(noise=-1)): pairwise F / precision / recall, BCubed F, the number of clusters and
        the number of noise items.  Thresholds are similarities with the conversion and the 'opt' of `_cluster`."""
        db = self.config.get('dbscan')
        if db is None:
            return {}
        db = dict(db)
        thrs, ms = list(db.get('thresholds', ())), db.get('min_samples', 4)
        dt = torch.float32 if not emb.is_cuda else getattr(self.config, 'match_dtype', torch.bfloat16)
        stats = []
        for t in thrs:
            sim = float(ps.opt_threshold()) if isinstance(t, str) and t == 'opt' else float(t)
            stats.append(M.ClusterStats(dbscan(emb, 2.0 * sim - 1.0, min_samples=ms, compute_dtype=dt), classes, noise=-1))
        out = {}
        out.update((f'DBSCAN F thr={t}', st.pairwise()[2]) for t, st in zip(thrs, stats))
        out.update((f'DBSCAN precision thr={t}', st.pairwise()[0]) for t, st in zip(thrs, stats))
        out.update((f'DBSCAN recall thr={t}', st.pairwise()[1]) for t, st in zip(thrs, stats))
        out.update((f'DBSCAN BCubed F thr={t}', st.bcubed()[2]) for t, st in zip(thrs, stats))
        out.update((f'DBSCAN clusters thr={t}', st.clusters) for t, st in zip(thrs, stats))
        out.update((f'DBSCAN noise thr={t}', st.noise) for t, st in zip(thrs, stats))
        return out

    def _open_set(self, emb, classes):
        """Opt-in (config.open_set = dict(fpir=[0.1, 0.01])): open-set identification of the set, every item searched against all the
        others (match.class_extremes: the match GEMM with a best-mate / best-impostor epilogue on the device; engine.metrics
        .OpenSetStats): 'OpenSet rank1', per false-positive identification rate f 'OpenSet DIR@FPIR={f}' (mated probes that come back at
        rank 1 at or above the threshold that alarms for at most f of the searches without a mate; FNIR = 1 - DIR) and 'OpenSet
        TH@FPIR={f}' (a similarity (cos + 1) / 2 like every TH@…), and 'OpenSet suspects', the number of items whose best impostor
        ranks before their best mate (match.label_suspects)."""
        cfg = self.config.get('open_set')
        if cfg is None:
            return {}
        fpirs = list(dict(cfg).get('fpir', (0.1, 0.01)))
        dt = torch.float32 if not emb.is_cuda else getattr(self.config, 'match_dtype', torch.bfloat16)
        ex = class_extremes(emb, classes, compute_dtype=dt, weakest=False)
        st = M.OpenSetStats(ex.pos_score, ex.pos_index, ex.neg_score, ex.neg_index)
        out = {'OpenSet rank1': st.rank1()}
        out.update((f'OpenSet DIR@FPIR={f}', st.dir_at_fpir(f)) for f in fpirs)
        out.update((f'OpenSet TH@FPIR={f}', (st.threshold_at_fpir(f) + 1.0) / 2.0) for f in fpirs)
        out['OpenSet suspects'] = int(label_suspects(ex).numel())
        return out

    def _quality(self, emb, scores, labels, pair_generator):
        """Opt-in (config.quality = True): the embeddings' lengths as a quality score (match.embedding_quality; a MagFace head trains
        them): 'Quality mean norm', and 'Quality AUC', how well min(|a|, |b|) tells the high-scoring genuine pairs from the low-scoring
        ones (match.quality_report)."""
        if not self.config.get('quality'):
            return {}
        from ..match import quality_report
        ci = pair_generator.corrected_indices
        return quality_report(emb, scores, labels, [a for a, _ in ci], [b for _, b in ci])

    def test_epoch_end(self, outputs):
        all_metrics = {}
        for i in range(len(outputs)):
            emb, classes = self._gather(outputs[i])
            name, pair_generator = self.config.pair_generator(i)
            scores, labels = self._pair_scores(emb, pair_generator)
            ps = M.PairStats(scores, labels)
            metrics = {'ROC AUC': ps.auroc(), 'Accuracy': ps.best_threshold_accuracy()[0]}
            rk = self._recall(emb, classes, [10, 100])
            metrics.update({f'Recall@K={k}': (x / y if y else float('nan')) for k, (x, y) in rk.items()})
            metrics.update(self._all_pairs(emb, classes))
            metrics.update(self._rerank_recall(emb, classes, [10, 100]))
            metrics.update(self._retrieval(emb, classes))
            metrics.update(self._cluster(emb, classes, ps))
            metrics.update(self._dbscan(emb, classes, ps))
            metrics.update(self._open_set(emb, classes))
            metrics.update(self._quality(emb, scores, labels, pair_generator))
            metrics.update(self._align_rejected(outputs[i]))
            print('', *[f'{name} {k}\t{v}' for k, v in metrics.items()], sep='\n')
            all_metrics[name] = metrics
        self.last_metrics = all_metrics
        return all_metrics

    def validation_epoch_end(self, outputs):
        m = self._evaluate(outputs)
        if self.logger is not None and hasattr(self.logger, 'log_artifacts'):
            self.logger.log_artifacts(str(self.config.output))
        return m

    def _evaluate(self, outputs):
        """The metrics dict of the reference's `_evaluate` (controller.py:95-183): the same keys in the same order
        ('ROC AUC', 'AveragePrecision', 'Accuracy', 'Opt thr', f'Accuracy thr={thr}' / 'Precision thr=…' / 'Recall thr=…' over
        config.thrs, f'Recall@K={k}' over config.k, f'TAR@FAR={far}' + f'TH@FAR={far}', f'TRR@FRR={frr}' + f'TH@FRR={frr}') and the
        same threshold rules (engine/metrics.py) — pinned key for key to the reference's own run, tests/golden/evaluate.npz."""
        cfg = self.config
        all_metrics = {}
        self.last_confmat = {}
        rocs = []
        for i in range(len(outputs)):
            emb, classes = self._gather(outputs[i])
            name, pair_generator = cfg.pair_generator(i)
            scores, labels = self._pair_scores(emb, pair_generator)
            ps = M.PairStats(scores, labels)
            fpr, tpr, thr = ps.roc()
            opt_thr = ps.opt_threshold()
            cm = ps.stats_at(opt_thr)
            confmat = [[cm['tn'], cm['fp']], [cm['fn'], cm['tp']]]          # [target][prediction], torchmetrics.ConfusionMatrix
            print(name, f'\nConf Mat thr = {opt_thr}', confmat)
            metrics = {'ROC AUC': ps.auroc(), 'AveragePrecision': ps.average_precision(),
                       'Accuracy': ps.best_threshold_accuracy(thr, fpr, 1 - tpr)[0], 'Opt thr': opt_thr}
            thrs = cfg.get('thrs', ())
            at = [ps.stats_at(float(t)) for t in thrs]
            metrics.update((f'Accuracy thr={t}', st['accuracy']) for t, st in zip(thrs, at))
            metrics.update((f'Precision thr={t}', st['precision']) for t, st in zip(thrs, at))
            metrics.update((f'Recall thr={t}', st['recall']) for t, st in zip(thrs, at))
            ks = list(cfg.get('k', ()))
            if len(ks):
                rk = self._recall(emb, classes, ks)
                metrics.update({f'Recall@K={k}': (x / y if y else float('nan')) for k, (x, y) in rk.items()})
            for far, (tar, th) in ps.far_points(cfg.get('far_thr', ())).items():
                metrics[f'TAR@FAR={far}'] = tar
                metrics[f'TH@FAR={far}'] = th
            for frr, (trr, th) in ps.frr_points(cfg.get('frr_thr', ())).items():
                metrics[f'TRR@FRR={frr}'] = trr
                metrics[f'TH@FRR={frr}'] = th
            metrics.update(self._all_pairs(emb, classes))
            metrics.update(self._rerank_recall(emb, classes, ks))
            metrics.update(self._retrieval(emb, classes))
            metrics.update(self._cluster(emb, classes, ps))
            metrics.update(self._dbscan(emb, classes, ps))
            metrics.update(self._open_set(emb, classes))
            metrics.update(self._quality(emb, scores, labels, pair_generator))
            metrics.update(self._align_rejected(outputs[i]))
            all_metrics[name] = metrics
            self.last_confmat[name] = confmat
            print(*[f'{name} {k}\t{v}' for k, v in metrics.items()], sep='\n')
            self._plot_confmat(name, cm)
            self._log(name, metrics)
            rocs.append((fpr.numpy(), tpr.numpy(), metrics['ROC AUC'], name))
        self._plot_rocs(rocs)
        self.last_metrics = all_metrics
        return all_metrics

    # the two figures the reference's _evaluate writes per validation epoch (controller.py:185-203); skipped when matplotlib
    # is not installed
    def _img_dir(self):
        d = Path(self.config.get('img_dir', '.'))
        d.mkdir(parents=True, exist_ok=True)
        return d

    def _plot_confmat(self, name, cm):
        try:   # an Agg canvas of its own: library code must not switch the process-wide matplotlib backend
            from matplotlib.figure import Figure
            from matplotlib.backends.backend_agg import FigureCanvasAgg
        except ImportError:
            return
        mat = [[cm['tn'], cm['fp']], [cm['fn'], cm['tp']]]
        fig = Figure()
        FigureCanvasAgg(fig)
        ax = fig.subplots()
        ax.imshow(mat, cmap='viridis')
        for r in range(2):
            for c in range(2):
                ax.text(c, r, str(mat[r][c]), ha='center', va='center', color='w')
        ax.set_xticks([0, 1]); ax.set_yticks([0, 1])
        ax.set_xlabel('Predicted label'); ax.set_ylabel('True label')
        fig.savefig(self._img_dir() / f' {name}_confmat_{self.current_epoch}.png')

    def _plot_rocs(self, rocs):
        try:
            from matplotlib.figure import Figure
            from matplotlib.backends.backend_agg import FigureCanvasAgg
        except ImportError:
            return
        fig = Figure(figsize=(10, 10))
        FigureCanvasAgg(fig)
        ax = fig.subplots()
        for fpr, tpr, auc, name in rocs:
            ax.plot(fpr, tpr, label=f'{name} AUC = {auc}', linewidth=3)
        ax.plot([0, 1], [0, 1], 'k--', linewidth=3)
        ax.set_xlabel('False positive rate'); ax.set_ylabel('True positive rate')
        ax.set_title('ROC curves'); ax.grid(); ax.legend()
        fig.savefig(self._img_dir() / f'roc_{self.current_epoch}.png')

    def _log(self, name, metrics):
        if self.logger is not None and hasattr(self.logger, 'log_metrics'):
            self.logger.log_metrics({f'{name} {k}': v for k, v in metrics.items()}, step=self.current_epoch)
        out = self.config.get('output', None)
        if out is not None:
            try:
                Path(out).mkdir(parents=True, exist_ok=True)
                with open(Path(out) / 'metrics.jsonl', 'a') as f:
                    f.write(json.dumps({'time': time.time(), 'epoch': self.current_epoch, 'set': name, **metrics}) + '\n')
            except OSError:
                pass

    @staticmethod
    def compute_accuracy(scores, labels, thresholds, fpr, fnr):
        return M.best_threshold_accuracy(scores, labels, thresholds, fpr, fnr)[0]

    # ------------------------------------------------------------------ delegation to the config
    def train_dataloader(self):
        return self.config.train_dataloader()

    def val_dataloader(self):
        return self.config.val_dataloader()

    def test_dataloader(self):
        return self.config.test_dataloader() if 'test_dataloader' in self.config else self.config.val_dataloader()

    def configure_optimizers(self):
        return self.config.optimizer(self.model_loss)
