"""Shared by the GPU suites that hold kernels to repeatability under load (tests/test_lds_pipeline_gpu.py,
tests/test_attn_bound_gpu.py)."""
import torch


def _repeat_under_load(dev, fns):
    """every fn() 12 times, bit-identical to its first result, with a side stream adding to 256 MB and the L2 evicted every
    third iteration"""
    first = [tuple(t.clone() for t in f()) for f in fns]
    side = torch.cuda.Stream()
    big = torch.zeros(256 << 20, device=dev, dtype=torch.uint8)
    junk = torch.empty(1 << 28, device=dev, dtype=torch.uint8)
    side.wait_stream(torch.cuda.current_stream())
    big.record_stream(side)
    try:
        for it in range(12):
            if it % 3 == 0:
                junk.fill_(it)  # evict L2 / Infinity Cache
            with torch.cuda.stream(side):
                for _ in range(4):
                    big.add_(1)   # HBM-bound traffic beside the kernels
            for k, f in enumerate(fns):
                for a, b in zip(f(), first[k]):
                    assert torch.equal(a, b), (k, it)
    finally:
        torch.cuda.synchronize()   # (no side-stream write outlives the test, also when an assert ends it)
