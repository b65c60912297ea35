"""Shared builder for the synthetic FE configs.  The config CONTRACT is the reference's
(/root/reference/configs/dog_fe/fe_dogs_config.py:67-162): model(), loss(config, model_), optimizer(model_),
train_dataloader(), val_dataloader(), pair_generator(idx), similarity_f(pairs), n_epochs, thrs, far_thr, k,
trainer_kwargs, output, device, distributed_train, world_size.  Data are synthetic (datasets need downloads)."""
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader

import models
from data_loading import SyntheticRecDataset, RecSubset, PairGenerator
from losses import SoftmaxBasedMetricLearning, PairMetricLearning



def _rank():
    """data-parallel rank of this process (torchrun), 0 otherwise: the reference's dataloader workers draw their augmentation
    decisions from per-worker / per-rank seeds, so the ranks must not share one decision stream"""
    import os
    return int(os.environ.get("RANK", "0"))

def _live(key, default):
    """value of `key` in the live Config object (main.py's batch-size / lr finders write there), else the config file's own"""
    from utils import Config, _SingletonBase
    inst = _SingletonBase._instances.get(Config)
    v = inst.get(key) if inst is not None else None
    return default if v is None else v


def make(ns, arch, n_train_ids, n_val_ids, photos, image_size, train_bs, test_bs, device, n_epochs=1, seed=0,
         fused_optimizer=True, compute_dtype=None, limit_train_batches=None, workers=0, n_pairs=200, device_augment=False, noise=0.15,
         noise_bank=0, limit_val_batches=None, gradient_clip_val=None, gradient_clip_algorithm=None, loss_kwargs=None, is_focal=True,
         ragged=False, pipeline='head', trainer_extra=None, model_kwargs=None, optimizer_kind='sgd', sub_centers=1, augment_extra=None, margin=None,
         margin_kwargs=None, sample_rate=None, sparse_grad=None, align=None, pair_loss=None, pk=None, centre_free=False):
    # pair_loss: dict(kind='supcon' | 'circle' | 'batch_hard' | 'multi_similarity', weight=1.0, **params) adds a pair loss on the batch's Gram matrix (losses/pair.py) to the head's
    # loss; with centre_free=True there is no class head at all and the pair loss is the criterion (losses.PairMetricLearning)
    # pk: (P, K) draws the train batches as P identities x K photos (data_loading.PKBatchSampler; train_bs is then P * K) so that every
    # anchor has positives; None = the reference's shuffled batches
    if centre_free and pair_loss is None:
        raise ValueError("centre_free=True trains on the pair loss alone: pass pair_loss=dict(kind=...)")
    # align: dict(jitter=…, estimate=…, masks=…) puts the landmark alignment (data_loading/align.py, the reference's preprocessor/align.py) in front
    # of the head pipeline: ragged raw frames + three landmarks -> DeviceAlign(base_pts, (image_size, image_size, 3)) -> the head augmentation
    # sample_rate / sparse_grad: Partial FC in the margin head (losses/large_margin.py); None = every class is scored, as in the reference
    # augment_extra: further DeviceAugmentation keywords of the train pipeline (p_hflip, color_jitter, p_grayscale, erasing); None = the reference's pipeline
    if augment_extra and not device_augment:
        raise ValueError("augment_extra configures the device pipeline (device_augment=True)")
    # margin / margin_kwargs: 'adaface' / 'curricular' replace the ArcFace head (losses/large_margin.py); None = the reference's head
    # sub_centers: K centres per class in the margin head (losses/large_margin.py); 1 = the reference's head
    # optimizer_kind: 'sgd' (the reference's SGD + MultiStepLR) or 'adamw' (FusedAdamW on the device, torch.optim.AdamW on the CPU)
    if optimizer_kind not in ('sgd', 'adamw'):
        raise ValueError(f"optimizer_kind must be 'sgd' or 'adamw', got {optimizer_kind!r}")
    # pipeline: which of the reference's three Compose shapes runs on the device (data_loading/augment.py): 'head' (uniform frames),
    # 'simple' / 'body' (ragged frames: the detector's raw crops, each with its own size)
    if pipeline not in ('head', 'simple', 'body'):
        raise ValueError(f"pipeline must be 'head', 'simple' or 'body', got {pipeline!r}")
    if align is not None and not (ragged and device_augment and pipeline == 'head'):
        raise ValueError("align reads ragged frames and hands uniform ones to the 'head' pipeline (ragged=True, device_augment=True, pipeline='head')")
    if (pipeline != 'head') != (bool(ragged) and align is None) or (ragged and not device_augment):
        raise ValueError("the 'simple' and 'body' pipelines read ragged frames (ragged=True, device_augment=True); 'head' reads uniform ones")
    torch.manual_seed(seed)
    dataset = SyntheticRecDataset(n_train_ids + n_val_ids, photos, image_size, seed=seed, noise=noise, raw_uint8=device_augment,
                                  noise_bank=noise_bank, **({'ragged': True} if ragged else {}),
                                  **({'landmarks': True, 'masks': bool(align.get('masks'))} if align is not None else {}))
    collate = {}
    if ragged:
        from data_loading import ragged_collate
        collate = {'collate_fn': ragged_collate}
    train_users = list(range(n_train_ids))
    val_users = list(range(n_train_ids, n_train_ids + n_val_ids))
    labels = dataset.get_labels()
    train_idx = [i for i, u in enumerate(labels) if u < n_train_ids]
    val_idx = [i for i, u in enumerate(labels) if u >= n_train_ids]
    assert not (set(train_users) & set(val_users))
    train, val = RecSubset(dataset, train_idx), RecSubset(dataset, val_idx)
    n_pairs = min(n_pairs, n_val_ids * photos * (photos - 1))   # the reference asserts gen_number <= #ordered genuine pairs
    pair_gen = PairGenerator(dataset, n_pairs, 1, None, seed, val_users)

    def pair_generator(idx):
        if idx in (0, 1):
            return ('Val', 'Val 1')[idx], pair_gen
        raise Exception

    def similarity_f(pairs):
        t1 = torch.stack([p[0] for p in pairs])
        t2 = torch.stack([p[1] for p in pairs])
        return (F.cosine_similarity(t1, t2) + 1) / 2

    similarity_f._is_default_cosine = True   # lets the evaluator use the fused HIP pair-score kernel

    def model():
        kw = {} if compute_dtype is None else {'compute_dtype': compute_dtype}
        if arch.startswith('swin'):   # the reference's own backbone (models/swin.py:228-241): `mlp_head` IS the 512-d embedding layer
            return getattr(models, arch)(num_classes=512, **kw)
        if arch.startswith('convnext'):   # masked_head_dog.py:105-106: `model_.classifier[2] = torch.nn.Linear(768, 512)`
            model_ = getattr(models, arch)(**kw, **(model_kwargs or {}))
            model_.classifier[2] = torch.nn.Linear(model_.classifier[2].in_features, 512)
            return model_
        if arch.startswith('mobilenet'):   # fe_dogs_config.py:104-105: `model_.classifier = torch.nn.Sequential(torch.nn.Linear(model_.last_channel, 512))`
            model_ = getattr(models, arch)(**kw, **(model_kwargs or {}))
            model_.classifier = torch.nn.Sequential(torch.nn.Linear(model_.last_channel, 512))
            return model_
        if arch.startswith('efficientnet'):   # fe_dogs_config.py:105-106: `model_.classifier = torch.nn.Linear(1408, 512)` (1408 = B2's last width)
            model_ = getattr(models, arch)(**kw, **(model_kwargs or {}))
            model_.classifier = torch.nn.Linear(model_.classifier[1].in_features, 512)
            return model_
        if arch.startswith('vit'):   # the FE line of a ViT backbone: `model_ = models.vit_b_16(); model_.heads = torch.nn.Linear(768, 512)`
            model_ = getattr(models, arch)(**kw, **(model_kwargs or {}))
            model_.heads = torch.nn.Linear(model_.hidden_dim, 512)
            return model_
        if arch.startswith('iresnet'):   # the face backbone: flatten → fc → features IS its 512-d embedding neck (models/iresnet.py)
            return getattr(models, arch)(num_features=512, **kw, **(model_kwargs or {}))
        model_ = getattr(models, arch)(**kw)
        model_.fc = torch.nn.Linear(model_.fc.in_features, 512)
        return model_

    def loss(config, model_):
        _ = config
        # loss_kwargs go to FocalLoss (is_focal) or nn.CrossEntropyLoss as in the reference (losses/__init__.py:28-33).  A learnable
        # FocalLoss alpha is in no optimizer group below, as in the reference's configs: it stays at its initial ones unless a config adds it.
        # margin / margin_kwargs are passed on only when set, so that the other configs build exactly the head they did
        margin_args = {}
        if margin is not None:
            margin_args['margin'] = margin
        if margin_kwargs is not None:
            margin_args['margin_kwargs'] = margin_kwargs
        if sample_rate is not None:
            margin_args['sample_rate'] = sample_rate
        if sparse_grad is not None:
            margin_args['sparse_grad'] = sparse_grad
        if centre_free:
            return PairMetricLearning(model=model_, pair_loss=pair_loss, embedding_size=512)
        if pair_loss is not None:
            margin_args['pair_loss'] = pair_loss
        return SoftmaxBasedMetricLearning(model=model_, num_class=n_train_ids, embedding_size=512, is_focal=is_focal,
                                          loss_kwargs=loss_kwargs, arc_margin=True, sub_centers=sub_centers, **margin_args)

    def optimizer(model_):
        # the reference's backbone / embedding-layer split ('fc'); the embedding layer of the torchvision-style backbones is `classifier` / `heads`
        head = 'classifier' if arch.startswith(('convnext', 'mobilenet', 'efficientnet')) else ('heads' if arch.startswith('vit') else 'fc')
        heads = ('fc.', 'features.') if arch.startswith('iresnet') else (head,)   # IResNet: the Linear and the BatchNorm1d behind it
        params1 = [p for i, p in model_.module.named_parameters() if not any(h in i for h in heads)]
        params2 = [p for i, p in model_.module.named_parameters() if any(h in i for h in heads)]
        base = _live('init_lr', 10 ** -2 if optimizer_kind == 'sgd' else 10 ** -3)
        d = [{'lr': base / 2, 'params': params1},
             {'lr': base, 'params': params2},
             {'lr': base, 'params': list(model_.add_margin.parameters()) if hasattr(model_, 'add_margin') else [], 'weight_decay': 1 * (10 ** -4)}]
        d = [g for g in d if len(g['params'])]   # (a backbone without an `fc` layer — Swin's embedding layer is `mlp_head` — has no second group)
        if optimizer_kind == 'adamw':
            if fused_optimizer and device != 'cpu':
                from optim import FusedAdamW
                optim = FusedAdamW(d, base, weight_decay=0.05)
            else:
                optim = torch.optim.AdamW(d, base, weight_decay=0.05)
        elif fused_optimizer and device != 'cpu':
            from optim import FusedSGD
            optim = FusedSGD(d, 0.01, momentum=0.9)
        else:
            optim = torch.optim.SGD(d, 0.01, momentum=0.9)
        sched = torch.optim.lr_scheduler.MultiStepLR(optim, milestones=[35, 45], gamma=0.1)
        return [optim], [sched]

    pk_epoch = [0]

    def train_dataloader():
        # pinned batches for the copy stream (data_loading/prefetch.py); workers stay alive across epochs like the reference's
        # persistent_workers loaders (fe_dogs_config.py:135-143)
        # (batch size and the base rate are read from the config namespace at call time: main.py's find_max_batch_size /
        # find_optimal_init_lr write train_batch_size / init_lr there, reference main.py:79-89)
        if pk is not None:
            # P identities x K photos per batch; a fresh, reproducible order per epoch (the loader is built once per epoch)
            from data_loading import PKBatchSampler
            sampler = PKBatchSampler([labels[i] for i in train_idx], pk[0], pk[1], seed=seed + _rank())
            sampler.set_epoch(pk_epoch[0])
            pk_epoch[0] += 1
            return DataLoader(train, batch_sampler=sampler, num_workers=workers, pin_memory=device != 'cpu',
                              persistent_workers=workers > 0, prefetch_factor=4 if workers > 0 else None, **collate)
        return DataLoader(train, _live('train_batch_size', train_bs), shuffle=True, drop_last=True, num_workers=workers, pin_memory=device != 'cpu',
                          persistent_workers=workers > 0, prefetch_factor=4 if workers > 0 else None, **collate)

    def val_dataloader():
        return DataLoader(val, _live('test_batch_size', test_bs), num_workers=0, **collate)

    if align is not None:
        from data_loading import DeviceAlign
        base_pts, dsize = dataset.base_pts((image_size, image_size)), (image_size, image_size, 3)
        kw = dict(estimate=align.get('estimate', 'reference'), min_distance=align.get('min_distance', 5.0))
        ns['device_align'] = DeviceAlign(base_pts, dsize, **kw)
        if align.get('jitter'):    # landmark jitter is a training augmentation: the validation frames are aligned on the landmarks as given
            ns['device_train_align'] = DeviceAlign(base_pts, dsize, jitter=align['jitter'],
                                                   generator=torch.Generator().manual_seed(seed + 7919 * (_rank() + 1)), **kw)
    if device_augment and pipeline != 'head':
        # simple_fe_dog.py:17-31 / body_dog_fe.py:18-33 on ragged batches, at this config's network input size
        from data_loading import DeviceAugmentation
        gen = torch.Generator().manual_seed(seed + _rank())
        hw, crop = (image_size, image_size), (image_size - 4, image_size - 4)
        fit, order = (('resize', hw), 'color_first') if pipeline == 'simple' else (('thumbnail_pad', hw), 'geometry_first')
        ns['device_train_augmentation'] = DeviceAugmentation(crop, hw, 0.1, 0.3, 5.0, gen, fit=fit, order=order, **(augment_extra or {}))
        ns['device_val_augmentation'] = DeviceAugmentation(None, None, 0.0, 0.0, 0.0, fit=fit)
    elif device_augment:
        # the reference's train/val Compose pipelines (fe_dogs_config.py:17-32) applied on the device to uint8 batches
        from data_loading import DeviceAugmentation, val_augmentation
        ns['device_train_augmentation'] = DeviceAugmentation((image_size - 4, image_size - 4), (image_size, image_size), 0.1, 0.3,
                                                             5.0, torch.Generator().manual_seed(seed + _rank()), **(augment_extra or {}))
        ns['device_val_augmentation'] = val_augmentation()
    # the reference's commented-out `gradient_clip_val=1, gradient_clip_algorithm='norm'` trainer_kwargs (fe_dogs_config.py:146-147):
    # passed on only when set, so that the other configs build exactly the trainer they did
    clip_kwargs = {}
    if gradient_clip_val is not None:
        clip_kwargs['gradient_clip_val'] = gradient_clip_val
    if gradient_clip_algorithm is not None:
        clip_kwargs['gradient_clip_algorithm'] = gradient_clip_algorithm
    output = Path('results')
    output.mkdir(exist_ok=True)
    ns.update(dict(
        n_epochs=n_epochs, train_batch_size=train_bs, test_batch_size=test_bs,
        thrs=np.linspace(0.5, 0.99, 6), far_thr=[0.1, 0.05, 0.03, 0.01, 0.005, 0.001], k=[5, 10, 100],
        pair_generator=pair_generator, similarity_f=similarity_f, model=model, loss=loss, optimizer=optimizer,
        train_dataloader=train_dataloader, val_dataloader=val_dataloader,
        trainer_kwargs=dict(benchmark=True, limit_train_batches=limit_train_batches, limit_val_batches=limit_val_batches,
                            **clip_kwargs, **(trainer_extra or {})),
        output=output, experiment_name='Synthetic', run_name=f'{arch} synthetic',
        device=device, distributed_train=not isinstance(device, str),
        world_size=len(device) if not isinstance(device, str) else None))
