"""A forked child never finalises what it inherited: an unreachable cycle that existed at the fork (in the product: one that owns a
hipGraph, an event or a host window) must be left to the parent, which owns the resources -- the child has no GPU runtime to release
them with.  No GPU needed: the finaliser here writes a byte into a pipe."""
import gc
import os


def test_a_forked_child_leaves_inherited_garbage_to_the_parent():
    import rlgym_ppo_amd  # noqa: F401  (registers the after-fork hook)
    r, w = os.pipe()

    class Owner:
        def __del__(self):
            os.write(w, b"x")

    was_enabled = gc.isenabled()
    gc.disable()
    try:
        a, b = Owner(), Owner()
        a.other, b.other = b, a
        del a, b                                   # an unreachable cycle, not yet collected
        pid = os.fork()
        if pid == 0:
            try:
                gc.collect()                       # what an allocation in the child would start sooner or later
            finally:
                os._exit(0)
        assert os.waitpid(pid, 0)[1] == 0
        os.set_blocking(r, False)
        try:
            seen = os.read(r, 16)
        except BlockingIOError:
            seen = b""
        assert seen == b"", "the forked child ran finalisers of objects it inherited"
        gc.collect()                               # the parent collects and releases as always
        assert os.read(r, 16) == b"xx"
    finally:
        if was_enabled:
            gc.enable()
        os.close(r)
        os.close(w)
