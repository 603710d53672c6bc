"""What the plan-backed detectors (HipDetector, HipGflDetector) share: the LRU cache of compiled plans, the hipGraph
capture of a plan, and the replay of one.  torch and the HIP library are imported where they are used, not here: the
cache is plain Python and is tested without a GPU."""
from __future__ import annotations

import os
import threading


class PlanCache:
    """key -> compiled plan, least recently used first.  Looked up, touched and evicted by several lanes' threads."""

    def __init__(self):
        self.entries = {}
        self.lock = threading.Lock()

    def get(self, key, build):
        """The plan of `key`; build() makes it on a miss.  build() runs outside the lock: two threads asking for the same
        key at once both build; the second insert wins, the first plan is dropped: correct, rare."""
        with self.lock:
            if key in self.entries:
                self.entries[key] = self.entries.pop(key)      # most recently used last
                return self.entries[key]
        c = build()
        # LRU cap on resident plans (each holds its activations, an NMS workspace and, today, its own copy of the packed
        # weights): the UFPMP fine stage compiles one plan per padded mosaic shape and lane -- without a cap HBM grows with
        # every new shape over a data set.  GLSDET_MAX_PLANS (default 24) plans stay; evicted ones are rebuilt on demand.
        cap = int(os.environ.get("GLSDET_MAX_PLANS", "24"))
        with self.lock:
            self.entries[key] = c
            while len(self.entries) > max(1, cap):
                self.entries.pop(next(iter(self.entries)))
        return c


class PlanBacked:
    """Base of the detectors: compile() of a subclass records its plan inside _plans.get(key, build) and ends build with
    _finish(c, use_graph); its run() hands its inputs (img, and img_hw / scale where it has them) to _replay."""

    def __init__(self):
        self._plans = PlanCache()
        self._compiled = self._plans.entries
        self._cache_lock = self._plans.lock

    @staticmethod
    def _finish(c, use_graph: bool):
        """Persist what the autotuner learnt while c.plan was recorded and, use_graph, capture the plan as one hipGraph on
        a private stream (c.graph_stream; None without a graph)."""
        import torch
        from . import _lib
        eng = c.eng
        eng.save_tune_cache()
        c.graph_stream = None
        if use_graph:
            # one capture at a time, and no device-wide synchronisation around it: another host thread (a lane of
            # the two-stage pipeline) may be capturing or launching -- a hipDeviceSynchronize issued while any
            # stream captures invalidates that capture
            with _lib.CAPTURE_LOCK:
                c.plan.run()                     # warm-up outside capture (lazy module load, attributes)
                torch.cuda.current_stream(eng.device).synchronize()
                c.graph_stream = torch.cuda.Stream(device=eng.device)
                with torch.cuda.stream(c.graph_stream):
                    c.plan.capture(c.graph_stream)
                c.graph_stream.synchronize()
        return c

    @staticmethod
    def _replay(c, stream=None, **inputs):
        """Copy the inputs that are not None into the plan's buffers of the same name (c.img, c.img_hw, c.scale), then one
        forward (+ post-processing if compiled in).  Asynchronous; a captured plan is replayed on its own stream, ordered
        after/before the caller's current stream."""
        import torch

        def feed():
            for name, t in inputs.items():
                if t is not None:
                    getattr(c, name).copy_(t, non_blocking=True)
        if c.plan.captured:
            st, cur = c.graph_stream, torch.cuda.current_stream()
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                feed()
                c.plan.launch(st)
            cur.wait_stream(st)
            return
        feed()
        c.plan.run(stream)

    @staticmethod
    def run_async(c):
        """Replay a captured plan on ITS OWN stream without ordering it against the caller's
        current stream: with two instances alternating, the latency-bound tail of batch i
        (NMS, small convs) overlaps the MFMA-bound body of batch i+1.  The caller synchronises
        (torch.cuda.synchronize() or c.graph_stream.synchronize()) before reading results."""
        assert c.plan.captured, "run_async needs compile(..., use_graph=True)"
        c.plan.launch(c.graph_stream)
