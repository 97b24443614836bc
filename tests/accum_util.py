"""Gradient accumulation restated in numpy float32 (rsu.h rsu_grad_accumulate, UNet.accumulate_gradients, UNet.dropout_key): what the
device tests compare against, bit for bit. No GPU, no library."""
import numpy as np

f32 = np.float32


def host_accumulate(dst, src, assign):
    """one call of the pass: dst = src (dst is not looked at), or dst + src with one float32 rounding per element"""
    src = np.asarray(src, f32)
    if assign:
        return src.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(dst, f32) + src).astype(f32)


def host_sum(grads):
    """what flat_g holds after the K-th accumulate_gradients(): ((g_0 + g_1) + ...) + g_{K-1}, every addition rounded to float32. The
    last call adds g_{K-1} + sum; float32 addition commutes, so that order changes no bit (a nan's payload aside)."""
    grads = [np.asarray(g, f32) for g in grads]
    acc = host_accumulate(None, grads[0], True)
    for g in grads[1:]:
        acc = host_accumulate(acc, g, False)
    return acc


def host_dropout_key(seed, site, global_step, micro_step=0):
    """the 32-bit dropout key: today's three terms, plus micro_step times an odd constant of its own"""
    return (seed * 0x9E3779B9 + site * 0x85EBCA6B + global_step * 0xC2B2AE35 + micro_step * 0x27D4EB2F) & 0xFFFFFFFF


def bits(a):
    """the float32 bit patterns of an array or of a (device) tensor"""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a), dtype=f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))
