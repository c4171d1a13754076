"""HIP-graph replay of a decode loop's device function: what ``vanilla_step``, ``lookup_round`` and the tree rounds share.

A loop (``llama_glide.py``) keeps its policy -- when a call is eligible, what its keys are, the hints of an eager call, whether
a failure switches ``use_graphs`` off -- and leaves to ``GraphReplayer`` the round driver (``run``: warm-up, capture, replay), the
capture stream, the memory pool, the tier a capture is sized for, the entries per key, the counters and what happens when any
of it fails."""
from __future__ import annotations

import warnings
from contextlib import contextmanager

import torch

_pinned = {}             # device index -> (graph, cell) that pin the generator's capture state, or the exception that kept them from it


def _pin_generator_state(stream):
    """torch creates the capture state of a device's default generator -- two one-element tensors that every capture and every
    replay fills in place -- at the first capture, and drops it when the last graph dies.  The loops capture inside
    ``torch.inference_mode``: created there the state is a pair of inference tensors, and a capture or a replay OUTSIDE
    inference mode (a caller's own graph around an operator, as the operator tests take) fails on that in-place update for as
    long as one of the loops' graphs is alive -- which the garbage collector decides.  One tiny graph captured outside
    inference mode in front of a device's first capture here, and kept for the life of the process, pins the state as ordinary
    tensors, which both modes may update.  Never replayed.  ``stream``: the capture stream of the caller; only a device's real
    stream has a generator behind it.  Best effort: a failure leaves everything as it was, and the loop's own capture, which
    follows, reports what it meets."""
    if not isinstance(stream, torch.Stream) or stream.device_index in _pinned:
        return
    _pinned[stream.device_index] = None
    try:
        with torch.inference_mode(False), torch.cuda.device(stream.device_index):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                cell = torch.zeros(1, device="cuda")
        _pinned[stream.device_index] = (graph, cell)
    except Exception as e:               # noqa: BLE001
        _pinned[stream.device_index] = e     # kept for whoever asks why; one warning, the loops go on as before this existed
        warnings.warn(f"the generator's capture state could not be pinned outside inference mode ({type(e).__name__}: {e})")


class GraphReplayer:
    """Entries per key: absent, ``"warm"`` (the device function has run once on the capture stream: the operator layer's
    workspaces are per stream, and lazy one-time work -- weight packing, kernel attributes -- must not fall into a capture)
    or ``(graph, result, workspace keep-alive)``.

    ``model`` provides ``_tier_bound`` / ``_set_hints`` / ``ops``, looked up at every call; ``hints(bound)`` is the pair of
    KV-length bounds of a launch sized for ``bound`` emitted tokens of ``total``; ``what`` names the device function in the
    warning; ``share_pool``: the captures of all keys allocate from one memory pool."""

    def __init__(self, model, hints, total: int, what: str, bound: int = 0, tiers: int = 0, share_pool: bool = False):
        self.model, self.hints, self.total, self.what, self.share_pool = model, hints, total, what, share_pool
        self.bound, self.tiers, self.captures = bound, tiers, 0
        self.entries, self.stream, self.pool = {}, None, None
        self.disabled = False            # after a failure: the loop runs eagerly from then on
        self.failed = False              # behind a guard: this call was the one that failed
        self.issued = False             # inside / behind a guard: this call's device work is already on the capture stream
        self.result = None               # ... and this is what it returned

    def roll_over(self, reached: int):
        """The generation has got to ``reached`` emitted tokens: past the tier the entries are sized for, drop them and
        size the next tier's."""
        if reached > self.bound:
            self.bound = self.model._tier_bound(reached, self.total)
            self.entries = {}
            self.tiers += 1

    def captured(self, key) -> bool:
        return isinstance(self.entries.get(key), tuple)

    def _set_hints(self):
        # grid bounds of the current tier, so that a capture stays valid until the generation leaves it
        self.model._set_hints(*self.hints(self.bound))

    def warm(self, key, device_fn):
        """Run ``device_fn`` eagerly ON the capture stream, sized like the capture that follows; returns its result."""
        cur = torch.cuda.current_stream()
        if self.stream is None:
            self.stream = torch.cuda.Stream()
        self._set_hints()
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self.result = device_fn()
        self.issued = True
        cur.wait_stream(self.stream)
        self.entries[key] = "warm"
        return self.result

    def capture(self, key, device_fn):
        self._set_hints()
        _pin_generator_state(self.stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self.stream, pool=self.pool):
            result = device_fn()
        if self.share_pool and self.pool is None:
            self.pool = graph.pool()
        # the graph holds raw pointers into the per-stream workspaces of the operator layer
        ops = self.model.ops
        keep = ops.workspace_tensors() if hasattr(ops, "workspace_tensors") else None
        self.entries[key] = (graph, result, keep)
        self.captures += 1

    def replay(self, key):
        graph, result, _ = self.entries[key]
        graph.replay()
        return result

    def run(self, key, device_fn, reached: int, same_call: bool = False):
        """One call of a loop on the graph path, the generation at ``reached`` emitted tokens: ``key`` absent -> warm-up,
        warm -> capture + replay, captured -> replay.  ``same_call`` (a loop with one key: the vanilla step, the lookup round)
        captures behind the warm-up in the call that warms; by default (one key per accepted count) the first call with a key
        warms and the second captures and replays.  Either way the warm-up IS the call's device work and never runs twice.
        Returns what ``device_fn`` returned, or None when the work has still to run, eagerly: after a failure (``failed``) in
        front of the warm-up -- tier sizing, ``wait_stream`` -- or in a replay."""
        with self.guard():
            self.roll_over(reached)
            if key not in self.entries:
                result = self.warm(key, device_fn)
                if same_call:
                    self.capture(key, device_fn)
                return result
            if not self.captured(key):
                self.capture(key, device_fn)
            return self.replay(key)
        return self.result if self.issued else None

    @contextmanager
    def guard(self):
        """Capture is an optimisation: an environment that cannot do it runs eagerly.  Any exception of the above inside this
        block (but one raised while a capture is open) becomes one warning, ``failed`` and ``disabled``; the block is left, and
        ``issued`` tells the caller whether the call's device work has run all the same (then ``result`` is its result, and
        the main stream has been made to wait for it) or is still to be done eagerly."""
        self.issued, self.result, self.failed = False, None, False
        try:
            yield
        except Exception as e:
            if torch.cuda.is_current_stream_capturing():
                raise
            warnings.warn(f"HIP-graph capture of the {self.what} failed ({type(e).__name__}: {e}); running eagerly")
            self.disabled = self.failed = True
            self.entries = {}
            if self.issued:
                torch.cuda.current_stream().wait_stream(self.stream)
