"""Dynamic batching for served torch models.

Triton-style request coalescing (the reference's ModelDynamicBatching
config, model_config.proto / SURVEY.md §2.7): concurrent requests are
merged along the batch dimension up to ``preferred_batch_size`` (or
until ``max_queue_delay_us`` expires), executed as one forward, and the
outputs are split back per request. Only requests with the same number
of tensors, dtypes and trailing shapes are merged; the first queued one
that differs (another sequence length, a request with an optional input
the others lack) ends the batch and opens the next. On the MI355X path both the gather
(torch.cat) and the scatter (slice copy_) are device-side — requests
arriving via HIP-shm never touch the host.
"""

import threading
import time


class DynamicBatcher:
    def __init__(self, model, preferred_batch_size=32, max_queue_delay_us=500,
                 max_batch_size=64):
        self._model = model
        self._preferred = preferred_batch_size
        self._delay_s = max_queue_delay_us / 1e6
        self._max = max_batch_size
        self._lock = threading.Lock()
        self._queue = []
        self._cv = threading.Condition(self._lock)
        self._worker = threading.Thread(target=self._run, daemon=True)
        self._alive = True
        self._worker.start()

    class _Item:
        __slots__ = ("tensors", "batch", "event", "outputs", "error",
                     "done_ev")

        def __init__(self, tensors, batch):
            self.tensors = tensors
            self.batch = batch
            self.event = threading.Event()
            self.outputs = None
            self.error = None
            self.done_ev = None  # hipEvent marking the batch's GPU work

    def infer(self, tensors):
        """Blocking: returns the list of output tensors for this request's
        slice. ``tensors`` batch dims must match across inputs."""
        outputs, ev = self.infer_async(tensors)
        if ev is not None:
            import torch

            # preserve the old contract: outputs are ordered on the
            # caller's current stream
            torch.cuda.current_stream().wait_event(ev)
        return outputs

    def infer_async(self, tensors):
        """Like infer, but returns (outputs, done_event). The batch runs
        on the batcher's OWN stream; done_event marks its completion.
        Callers order their consumption on the event instead of a full
        device sync — a per-request torch.cuda.synchronize() on the
        shared default stream was queueing each request's tiny output
        copy behind the NEXT batches' forwards (measured 5-6 ms
        avg_compute_output at c8)."""
        batch = tensors[0].shape[0]
        item = self._Item(tensors, batch)
        with self._cv:
            self._queue.append(item)
            self._cv.notify()
        if not item.event.wait(timeout=300):
            raise RuntimeError("dynamic batcher timed out")
        if item.error is not None:
            raise item.error
        return item.outputs, item.done_ev

    @staticmethod
    def _signature(tensors):
        """What two requests must share to be merged along dim 0: the
        number of tensors, their dtypes and their trailing shapes."""
        return tuple((t.dtype, tuple(t.shape[1:])) for t in tensors)

    def shutdown(self):
        with self._cv:
            self._alive = False
            self._cv.notify()

    def _run(self):
        import torch

        while True:
            with self._cv:
                while self._alive and not self._queue:
                    self._cv.wait()
                if not self._alive:
                    return
                items = [self._queue.pop(0)]
            # linger for more requests up to preferred/max or delay
            total = items[0].batch
            deadline = time.monotonic() + self._delay_s
            while total < self._preferred:
                remaining = deadline - time.monotonic()
                with self._cv:
                    if self._queue:
                        nxt = self._queue[0]
                        if total + nxt.batch > self._max:
                            break
                        if (self._signature(nxt.tensors)
                                != self._signature(items[0].tensors)):
                            # cannot be concatenated with this batch: it
                            # stays at the head for the next one
                            break
                        self._queue.pop(0)
                        items.append(nxt)
                        total += nxt.batch
                        continue
                if remaining <= 0:
                    break
                time.sleep(min(remaining, 0.0002))

            # NOTE: everything runs on the worker thread's DEFAULT
            # stream. A redesign that put batches on a dedicated stream
            # with event-gated output copies MEASURED SLOWER on MI355X
            # (ResNet 8569 -> 6167 inf/s, DenseNet 4648 -> 1638): the
            # single-stream pipeline is what the hardware runs best
            # here, and the per-request completion event below is
            # enough to avoid full-device syncs downstream.
            try:
                cuda = items[0].tensors and items[0].tensors[0].is_cuda
                if len(items) == 1:
                    outputs = self._model._execute_direct(items[0].tensors)
                    items[0].outputs = outputs
                else:
                    n_inputs = len(items[0].tensors)
                    merged = [
                        torch.cat([it.tensors[i] for it in items], dim=0)
                        for i in range(n_inputs)
                    ]
                    outputs = self._model._execute_direct(merged)
                    off = 0
                    for it in items:
                        it.outputs = [o[off : off + it.batch]
                                      for o in outputs]
                        off += it.batch
                done_ev = None
                if cuda:
                    # ring of reused events: creating one per batch
                    # churns HSA interrupt signals on ROCm (each
                    # hipEventCreate takes one); 64 deep is far beyond
                    # any consumer's lag
                    ring = getattr(self, "_ev_ring", None)
                    if ring is None:
                        ring = [torch.cuda.Event() for _ in range(64)]
                        self._ev_ring = ring
                        self._ev_idx = 0
                    done_ev = ring[self._ev_idx]
                    self._ev_idx = (self._ev_idx + 1) % len(ring)
                    done_ev.record()
                for it in items:
                    it.done_ev = done_ev
                    it.event.set()
            except Exception as e:  # pragma: no cover
                for it in items:
                    it.error = e
                    it.event.set()
