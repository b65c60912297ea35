"""P x K batches for the pair losses (losses/pair.py): every batch holds P identities with K items each, so that every anchor has K - 1
positives and (P - 1) K negatives.  A plain host class for DataLoader(batch_sampler=...)."""
import numpy as np


class PKBatchSampler:
    """PKBatchSampler(labels, P, K, seed=0, drop_last=True): yields lists of P * K dataset indices, K of each of P identities.

    Per epoch the identities are shuffled and cut into groups of P: an epoch shows every identity at most once (the last
    `n_ids % P` of the shuffle are left out: drop_last=True, the default) or, with drop_last=False, fills the last group up with the
    identities at the head of the same shuffle (which that group does not hold yet).  Of an identity with at least K items, K distinct
    ones are drawn; one with fewer is sampled WITH replacement (only then).  The order depends on (seed, epoch) alone: `set_epoch(e)`
    follows the DistributedSampler convention, the same (seed, epoch) gives the same batches on every call and every process (the loss is
    rank-local: ranks that want different batches give different seeds)."""

    def __init__(self, labels, P, K, seed=0, drop_last=True):
        labels = np.asarray(labels).reshape(-1)
        if P < 1 or K < 1:
            raise ValueError(f"PKBatchSampler: P and K must be >= 1, got P={P} K={K}")
        self.ids, inverse = np.unique(labels, return_inverse=True)
        if len(self.ids) < P:
            raise ValueError(f"PKBatchSampler: {len(self.ids)} identities cannot fill batches of P={P}")
        order = np.argsort(inverse, kind="stable")
        bounds = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(self.ids)))])
        self.items = [order[bounds[c]:bounds[c + 1]] for c in range(len(self.ids))]   # dataset indices per identity, ascending
        self.P, self.K, self.seed, self.drop_last, self.epoch = int(P), int(K), int(seed), bool(drop_last), 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        n = len(self.ids)
        return n // self.P if self.drop_last else (n + self.P - 1) // self.P

    def __iter__(self):
        rng = np.random.default_rng([self.seed, self.epoch])
        perm = rng.permutation(len(self.ids))
        P, K = self.P, self.K
        for b in range(len(self)):
            group = perm[b * P:(b + 1) * P]
            if len(group) < P:          # (drop_last=False only) the head of the shuffle holds none of this group's identities
                group = np.concatenate([group, perm[:P - len(group)]])
            batch = []
            for c in group:
                it = self.items[c]
                batch.extend(rng.choice(it, K, replace=len(it) < K).tolist())
            yield batch
