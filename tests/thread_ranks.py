"""Several ranks of a partition as threads of ONE process (tests only).

The GPU test machines are shared and allow only a few processes with the GPU open at a time, so a partition wider than
GPU_PROCS ranks cannot run one process per rank there.  `install()` replaces the torch.distributed calls the tests, the
host-staged transport (multigpu._HostTransport) and bench.py's multi-rank path make with in-process equivalents keyed by
the calling thread's rank; `run(world, fn)` then runs fn(rank) on `world` threads.  Point-to-point messages are FIFO per
(source, destination) pair as with gloo; every rank receives the same all-reduce result (summed in rank order).

The native library calls the host transport's callbacks on the thread that called it, so each callback sees its rank.  The
asynchronous host schedule (GMG_HOST_ASYNC=1) calls them from HIP's host-function thread instead: it needs a process per rank.

    python tests/thread_ranks.py W script.py args...    runs script.py's main() as W ranks (RANK / LOCAL_RANK per thread)
"""
import os
import queue
import sys
import threading

GPU_PROCS = 4                 # at most this many rank processes with the GPU open per test (plus the pytest process itself)
_WAIT_S = 1800.0              # a peer that has not answered by then has failed

_tls = threading.local()


class _World:
    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world, timeout=_WAIT_S)
        self.slots = [None] * world
        self.mail = {}
        self.lock = threading.Lock()
        self.failed = threading.Event()

    def box(self, src, dst):
        with self.lock:
            return self.mail.setdefault((src, dst), queue.Queue())

    def exchange(self, obj):
        """every rank's obj, in rank order, on every rank"""
        r = _rank()
        self.slots[r] = obj
        self.barrier.wait()
        out = list(self.slots)
        self.barrier.wait()            # nobody overwrites a slot before everyone has read it
        return out


_W = None


def _rank():
    return _tls.rank


class P2POp:
    def __init__(self, op, tensor, peer, group=None, tag=0):
        self.op, self.tensor, self.peer = op, tensor, peer


class _Done:
    def wait(self, *a, **k):
        return True

    def is_completed(self):
        return True


def isend(tensor, dst, group=None, tag=0):
    _W.box(_rank(), int(dst)).put(tensor.detach().clone())
    return _Done()


def irecv(tensor, src, group=None, tag=0):
    q = _W.box(int(src), _rank())
    while True:
        try:
            tensor.copy_(q.get(timeout=1.0))
            return _Done()
        except queue.Empty:
            if _W.failed.is_set():
                raise RuntimeError(f"rank {_rank()}: peer {src} failed")


def send(tensor, dst, group=None, tag=0):
    isend(tensor, dst)


def recv(tensor, src=None, group=None, tag=0):
    irecv(tensor, src)
    return src


def batch_isend_irecv(ops):
    for o in ops:                          # every send first: a receive never waits for a send this rank has yet to post
        if o.op is isend:
            isend(o.tensor, o.peer)
    for o in ops:
        if o.op is irecv:
            irecv(o.tensor, o.peer)
    return [_Done() for _ in ops]


def all_reduce(tensor, op=None, group=None, async_op=False):
    import torch
    import torch.distributed as dist
    parts = _W.exchange(tensor.detach().cpu().clone())
    acc = parts[0].clone()
    for p in parts[1:]:
        if op is None or op == dist.ReduceOp.SUM:
            acc += p
        elif op == dist.ReduceOp.MAX:
            acc = torch.maximum(acc, p)
        elif op == dist.ReduceOp.MIN:
            acc = torch.minimum(acc, p)
        else:
            raise NotImplementedError(f"all_reduce op {op}")
    tensor.copy_(acc.to(tensor.device))
    return _Done() if async_op else None


def all_gather_object(object_list, obj, group=None):
    object_list[:] = _W.exchange(obj)


def broadcast_object_list(object_list, src=0, group=None, device=None):
    object_list[:] = _W.exchange(list(object_list))[src]


def barrier(group=None, **k):
    _W.exchange(None)


def get_rank(group=None):
    return _rank()


def get_world_size(group=None):
    return _W.world


def get_global_rank(group, group_rank):
    return group_rank


def get_backend(group=None):
    return "gloo"


def init_process_group(*a, **k):
    pass


def destroy_process_group(*a, **k):
    pass


def is_initialized():
    return True


def new_group(*a, **k):
    return None


_NAMES = ("P2POp", "isend", "irecv", "send", "recv", "batch_isend_irecv", "all_reduce", "all_gather_object", "broadcast_object_list",
          "barrier", "get_rank", "get_world_size", "get_global_rank", "get_backend", "init_process_group", "destroy_process_group",
          "is_initialized", "new_group")


class _RankEnviron(type(os.environ)):
    """os.environ whose RANK / LOCAL_RANK are the calling rank thread's"""

    def __getitem__(self, key):
        if key in ("RANK", "LOCAL_RANK") and hasattr(_tls, "rank"):
            return str(_tls.rank)
        return super().__getitem__(key)


def install(world):
    """torch.distributed -> this module's in-process calls for `world` ranks (the whole process: ranks are its threads)"""
    global _W
    import torch
    import torch.distributed as dist
    if torch.cuda.is_available():          # once, here: torch's device queries are not safe against concurrent first callers
        torch.cuda.init()
        torch.cuda.device_count()          # (cached only from the first call after init)
    root =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import __graft_entry__ as entry
    entry.import_package().abi.load()      # once, before the rank threads would race to import and load it
    _W = _World(world)
    mod = sys.modules[__name__]
    for n in _NAMES:
        setattr(dist, n, getattr(mod, n))
    os.environ["WORLD_SIZE"] = str(world)
    os.environ.__class__ = _RankEnviron


def run(world, fn):
    """fn(rank) on `world` threads; the first failure (exception or SystemExit != 0) is re-raised here once all have stopped"""
    install(world)
    errors = [None] * world

    def body(r):
        _tls.rank = r
        try:
            fn(r)
        except SystemExit as e:
            if e.code not in (None, 0):
                errors[r] = e
        except BaseException as e:        # noqa: BLE001 -- reported below, after the peers are released
            errors[r] = e
        if errors[r] is not None:
            _W.failed.set()
            _W.barrier.abort()
    th = [threading.Thread(target=body, args=(r,), name=f"rank{r}") for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    bad = [(r, e) for r, e in enumerate(errors) if e is not None]
    if bad:
        first = next(((r, e) for r, e in bad if not isinstance(e, threading.BrokenBarrierError)), bad[0])
        import traceback
        for r, e in bad:
            sys.stderr.write(f"---- rank {r} ----\n" + "".join(traceback.format_exception(type(e), e, e.__traceback__)))
        raise SystemExit(f"rank {first[0]} failed: {first[1]!r}")


def _run_script(world, path, argv):
    """script's main() per rank thread, as if launched by torch.distributed.run with `world` processes"""
    import importlib.util
    sys.argv = [path] + argv
    sys.path.insert(0, os.path.dirname(os.path.abspath(path)))
    spec = importlib.util.spec_from_file_location("_ranked_main", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    if hasattr(mod, "claim_stdout"):
        mod.claim_stdout()                 # bench.py: once for the process, before the ranks race for it
    run(world, lambda r: mod.main())


if __name__ == "__main__":
    _run_script(int(sys.argv[1]), sys.argv[2], sys.argv[3:])
