#!/usr/bin/env python
"""FE evaluation entry point — counterpart of /root/reference/eval_fe_dog_head_sgd.py:9-27 and
eval_fe_cat_head_sgd.py: load config, optionally a reference-format `state_dict` (strict=False: the margin weight may
be stripped, download_models.py:8-9), run `trainer.test(controller)` → Controller.test_epoch_end (ROC AUC, Accuracy,
Recall@K=10/100)."""
import argparse
import os
import sys
from pathlib import Path

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
import pets_face_recognition_amd as pfr  # noqa: E402

pfr.install_reference_aliases()

import torch  # noqa: E402
from engine import Controller  # noqa: E402
from utils import configure_trainer, get_config  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('-c', '--config', required=True, type=Path)
    ap.add_argument('--checkpoint', type=Path, default=None, help='state_dict with keys model_loss.module.* (optional)')
    ap.add_argument('--averaged', action='store_true',
                    help="evaluate the checkpoint's averaged weights: `averaged_state_dict` of its .trainer sidecar (Trainer(ema_decay=))")
    ap.add_argument('--all-pairs-far', type=float, nargs='+', default=None, metavar='F',
                    help='also report verification metrics over EVERY pair of the set (score histograms from one GEMM): '
                         'AllPairs ROC AUC / EER and TAR, threshold at each of these false-accept rates, e.g. 1e-4 1e-5 1e-6')
    ap.add_argument('--rerank', nargs=3, default=None, metavar=('K1', 'K2', 'LAMBDA'),
                    help="also report 'Rerank Recall@K=…': Recall@K of the k-reciprocal re-ranked match lists (match.rerank), "
                         'e.g. 20 6 0.3')
    ap.add_argument('--retrieval', type=int, nargs='*', default=None, metavar='K',
                    help="also report the retrieval metrics 'mAP', 'mINP', 'CMC@K=…' and 'Mean first rank' from the exact rank of every "
                         'positive (match.positive_ranks); the CMC ranks K default to 1 5 10')
    ap.add_argument('--cluster', nargs='+', default=None, metavar='T',
                    help="also report 'Cluster F / precision / recall / BCubed F thr=…' and 'Clusters thr=…': identity clustering (single "
                         "linkage, match.cluster) at these similarity thresholds; 'opt' stands for the run's optimal threshold, e.g. 0.8 opt")
    ap.add_argument('--dbscan', nargs='+', default=None, metavar=('MIN_SAMPLES', 'T'),
                    help="also report 'DBSCAN F / precision / recall / BCubed F / clusters / noise thr=…': DBSCAN identity clustering "
                         "(match.dbscan) with MIN_SAMPLES items (the item itself included) per core neighbourhood at these similarity "
                         "thresholds; 'opt' stands for the run's optimal threshold, e.g. 4 0.8 opt")
    ap.add_argument('--open-set', type=float, nargs='+', default=None, metavar='F',
                    help="also report 'OpenSet rank1', 'OpenSet DIR@FPIR=F', 'OpenSet TH@FPIR=F' and 'OpenSet suspects': open-set "
                         "identification (match.class_extremes: every item searched against all the others) at these false-positive "
                         "identification rates, e.g. 0.1 0.01")
    ap.add_argument('--quality', action='store_true',
                    help="also report 'Quality mean norm' (mean length of the embeddings, match.embedding_quality) and 'Quality AUC' (how "
                         "well the smaller length of a genuine pair tells the high-scoring pairs from the low-scoring ones)")
    args = ap.parse_args(argv)
    config = get_config(args.config)
    if args.quality:
        config['quality'] = True
    if args.rerank is not None:
        config['rerank'] = dict(k1=int(args.rerank[0]), k2=int(args.rerank[1]), lambda_value=float(args.rerank[2]))
    if args.retrieval is not None:
        config['retrieval'] = dict(ks=list(args.retrieval) or [1, 5, 10])
    if args.cluster is not None:
        config['cluster'] = dict(thresholds=[t if t == 'opt' else float(t) for t in args.cluster])
    if args.dbscan is not None:
        if len(args.dbscan) < 2:
            ap.error('--dbscan needs MIN_SAMPLES and at least one threshold')
        config['dbscan'] = dict(thresholds=[t if t == 'opt' else float(t) for t in args.dbscan[1:]], min_samples=int(args.dbscan[0]))
    if args.open_set is not None:
        config['open_set'] = dict(fpir=list(args.open_set))
    if args.all_pairs_far is not None:
        config['all_pairs_far'] = list(args.all_pairs_far)
    controller = Controller(config)
    if args.averaged and args.checkpoint is None:
        ap.error('--averaged needs --checkpoint')
    if args.checkpoint is not None:
        if args.averaged:
            side = torch.load(str(args.checkpoint) + '.trainer', map_location='cpu')
            if 'averaged_state_dict' not in side:
                raise SystemExit(f'{args.checkpoint}.trainer holds no averaged_state_dict (was the run trained with ema_decay?)')
            sd = side['averaged_state_dict']
        else:
            sd = torch.load(args.checkpoint, map_location='cpu')
            sd = sd.get('state_dict', sd)
        missing, unexpected = controller.load_state_dict(sd, strict=False)
        print('loaded', args.checkpoint, 'missing', len(missing), 'unexpected', len(unexpected))
    trainer = configure_trainer(config, None, None)
    return trainer.test(controller)


if __name__ == '__main__':
    main()
