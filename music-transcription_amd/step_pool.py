"""Per-shape pools of training-step workspaces with a lease per step in flight (train_step.py: the BPTT hand-off workspaces,
train_step_large.py: the zero-padded step scratch).

A training step's forward pass hands its workspace to its own backward pass.  From the forward until that backward has run -- or
until the autograd graph holding the step is dropped without one -- the workspace is LEASED:
  * a second forward of the same shape gets a private workspace instead (two steps in flight, gradient accumulation);
  * eviction from the pool only ever drops idle entries; when every pooled entry is leased, a new shape gets a private workspace;
  * the lease is released by the end of the backward pass, by the no-grad path (no backward will follow), and by the lease's
    finaliser when the graph is garbage-collected without a backward (a skipped non-finite loss).

Why a release from the finaliser (at an arbitrary host time) is stream-safe: both training forwards join their side streams into
the calling stream before they return, so every use of the workspace is ordered on the calling stream ahead of anything the next
step enqueues there -- and the next step's own side-stream work starts behind an event recorded on the calling stream.  The same
holds for the release at the end of a backward pass, which joins its side streams the same way.  (As for the step in general:
consecutive steps of one model are issued on one calling stream.)

Pure Python (no GPU): the pool logic is tested on the CPU (tests/test_host_cpu.py)."""
from __future__ import annotations


class Lease:
    """Keeps `entry.busy` set until release() or until the lease itself is garbage-collected."""
    __slots__ = ("_entry",)

    def __init__(self, entry):
        entry.busy = True
        self._entry = entry

    def release(self) -> None:
        e, self._entry = self._entry, None
        if e is not None:
            e.busy = False

    def __del__(self):
        self.release()


def acquire(pool: dict, key, make, fresh, max_entries: int = 2):
    """-> (workspace, lease or None).  `pool` maps key -> entry (anything with a `busy` attribute, made by `make()`); at most
    `max_entries` shapes stay pooled (ragged batches: T varies).  The pooled entry for `key` comes back leased when it is idle;
    otherwise (leased by a step still in flight, or a full pool of leased entries) a private `fresh()` comes back without a lease."""
    e = pool.get(key)
    if e is None:
        for k in [k for k, v in pool.items() if not v.busy]:      # oldest first; never an entry a pending backward holds
            if len(pool) < max_entries:
                break
            del pool[k]
        if len(pool) >= max_entries:
            return fresh(), None
        e = pool[key] = make()
    if e.busy:
        return fresh(), None
    return e, Lease(e)


def release(sv: dict) -> None:
    """Releases the lease a training forward stored in its saved state (if any)."""
    lease = sv.get("lease")
    if lease is not None:
        lease.release()
