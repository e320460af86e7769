"""numpy restatement of the counter-based dropout mask of the HIP kernels (tqdne_amd/csrc/common.hpp: mix32, drop_key, drop_hash).
Element e = position * C + channel of sample b at dropout site `site` is KEPT iff drop_hash(drop_key(seed, site, b), e) >= threshold,
threshold = uint32(p * 2^32); kept values are multiplied by 1 / (1 - p) in fp32.

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).
"""

from __future__ import annotations

import numpy as np


def mix32(x):
    """csrc/common.hpp mix32 on numpy uint32 arrays (wrapping arithmetic)"""
    M = np.uint32
    x = np.asarray(x, dtype=np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> M(16)
        x *= M(0x7FEB352D)
        x ^= x >> M(15)
        x *= M(0x846CA68B)
        x ^= x >> M(16)
    return x


def drop_key(seed, site, b):
    """csrc/common.hpp drop_key: the per-sample key of dropout site ``site`` under the 64-bit ``seed``"""
    M = np.uint32
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    with np.errstate(over="ignore"):
        k = mix32(M(seed & 0xFFFFFFFF) ^ M(0x9E3779B9))
        k = mix32(k ^ M(seed >> 32))
        k = mix32(k + M(0x85EBCA6B) * M(site + 1))
        return mix32(k + M(0xC2B2AE35) * M(b + 1)), mix32((k ^ M(0x27D4EB2F)) + M(0x165667B1) * M(b + 1))


def drop_hash(key, e):
    """csrc/common.hpp drop_hash: the finaliser with the key's second word added between its two multiplies"""
    M = np.uint32
    ka, kb = key
    x = np.asarray(e, dtype=np.uint32) ^ ka
    with np.errstate(over="ignore"):
        x ^= x >> M(16)
        x *= M(0x7FEB352D)
        x += kb
        x ^= x >> M(15)
        x *= M(0x846CA68B)
        x ^= x >> M(16)
    return x


def dropout_scale_mask(seed, site, B, T, C, p):
    """(B, T, C) fp32 factors of a channels-last tensor at one site: 1 / (1 - p) where kept, 0 where dropped"""
    p32 = np.float32(p)
    thresh = np.uint32(int(float(p32) * 4294967296.0))
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    idx = np.arange(T * C, dtype=np.uint32)
    keep = np.stack([drop_hash(drop_key(seed, site, b), idx) >= thresh for b in range(B)])
    return np.where(keep, scale, np.float32(0)).astype(np.float32).reshape(B, T, C)
