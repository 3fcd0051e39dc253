"""Helpers shared by the GPU tests of the query families (test_gpu_fold_in, test_gpu_fold_in_batch, test_gpu_update,
test_gpu_revise): bit-for-bit comparison, the augmented train set, and the chunk rule of include/knncf.h."""
import numpy as np

UNKNOWN_ITEM = 999_999
MAX_CHUNK = 64


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64).tolist()


def _aug(train, q, items, ratings):
    u, i, r = train
    n = len(items)
    return (np.concatenate([u, np.full(n, q, dtype=np.int32)]).astype(np.int32),
            np.concatenate([i, np.asarray(items, dtype=np.int32)]).astype(np.int32),
            np.concatenate([r, np.asarray(ratings, dtype=np.float64)]))


def _same_pair(a, b, what):
    assert a[0].tolist() == b[0].tolist(), what
    assert _bits(a[1]) == _bits(b[1]), what


def _chunk(e, workspace_bytes):
    """the chunk rule of include/knncf.h for a handle created with workspace_bytes > 0"""
    per = 64 * e.num_users + 96 * e.num_items
    return max(1, min(MAX_CHUNK, (workspace_bytes // 2) // per, (2**31 - 1) // max(e.num_users, e.num_items)))


def _workspace_for(chunk, n_users, n_items):
    return 2 * chunk * (64 * n_users + 96 * n_items) + 2
