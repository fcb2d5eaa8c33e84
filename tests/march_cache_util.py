"""What the march cache's GPU test modules share (test_gpu_march_cache.py, test_gpu_march_cache_exits.py): the tests' budget and
views, an empty cache to count from, and the reference of every comparison -- the SAME launch with the device's cache configured
to 0 bytes (the uncached path: the single kernel), in the same process."""
import march_ref as mr

BUDGET = 2 << 30
VIEWS = {
    "bench": mr.VIEWS["default"],
    "key1": ((15.0, 3.0, -30.0), -20.0, -5.0),          # camera_paths.cpp:35
    "skimmer": mr.VIEWS["skimmer"],
    "in_disk": mr.VIEWS["in_disk"],
}


def fresh(rrt):
    """an empty cache with the tests' budget; returns the counters to take differences against"""
    rrt.march_cache_release()
    rrt.march_cache_configure(BUDGET)
    return rrt.march_cache_stats()


def delta(rrt, before):
    now = rrt.march_cache_stats()
    return {k: now[k] - before[k] for k in ("fills", "hits", "drops", "misses", "uncacheable")}


def frame(torch, n_bytes, fn):
    out = torch.zeros(n_bytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()              # the zeroing runs on the null stream; fn may launch on a non-blocking one
    fn(out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def uncached(rrt, fn):
    """fn() with the cache off; the cache comes back EMPTY with the tests' budget (configure forgets the key)"""
    rrt.march_cache_configure(0)
    try:
        return fn()
    finally:
        rrt.march_cache_configure(BUDGET)


def plain(torch, rrt, w, h, t, cam, tex, fx, prm, stream=None):
    return frame(torch, w * h * 4, lambda o: rrt.launch_raymarch(o, w, h, t, cam, tex, fx, prm, stream=stream))
