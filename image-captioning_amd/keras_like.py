"""The slice of the Keras Model / callbacks surface the reference's training scripts touch
(text_generation_model_v2.py:262-313, text_generation_model.py:424-472): compile, predict,
train_on_batch, test_on_batch, fit_generator, load_weights(by_name, skip_mismatch), save_weights,
trainable_weights, summary; ModelCheckpoint(save_weights_only) and CSVLogger."""
import csv
import os

import numpy as np
import torch

from . import ops, step_graph
from .params import get as get_optimizer
from .modified_dense_model import load_weight_file, save_weight_file


class ModelCheckpoint(object):
    """keras.callbacks.ModelCheckpoint(filepath, verbose, save_weights_only=True, mode='min'): the
    reference saves every epoch (save_best_only is left False), filename formatted with epoch/logs."""

    def __init__(self, filepath, verbose=0, save_weights_only=True, mode='min'):
        self.filepath, self.verbose = filepath, verbose

    def on_epoch_end(self, model, epoch, logs):
        path = self.filepath.format(epoch=epoch + 1, **logs)      # '.h5' names get Keras-layout HDF5 files, anything else .npz
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        model.save_weights(path)
        if self.verbose:
            print("Epoch %05d: saving model to %s" % (epoch + 1, path))


class CSVLogger(object):
    """keras.callbacks.CSVLogger(filename): epoch,<sorted log keys> rows."""

    def __init__(self, filename):
        self.filename, self._keys = filename, None

    def on_epoch_end(self, model, epoch, logs):
        os.makedirs(os.path.dirname(self.filename) or ".", exist_ok=True)
        new = self._keys is None
        if new:
            self._keys = sorted(logs)
        with open(self.filename, "w" if new else "a", newline="") as f:
            w = csv.writer(f)
            if new:
                w.writerow(["epoch"] + self._keys)
            w.writerow([epoch] + [logs[k] for k in self._keys])


def target_ids(y, ids_rank, vocab=None):
    """The targets of a Keras batch as int32 ids: y holds ids already (rank ids_rank: returned as int32, within [0, vocab) when vocab is
    given) or the one-hot rows of those ids along one more axis, as the reference's generators yield them (each row of width vocab, when
    given, and exactly one 1 among zeros)."""
    y = np.asarray(y)
    if y.ndim == ids_rank:
        if vocab is not None and y.size and (y.min() < 0 or y.max() >= vocab):
            raise ValueError("target ids must lie in [0, %d)" % vocab)
        return y.astype(np.int32)
    if (vocab is not None and y.shape[-1] != vocab) or not (np.all(y.max(-1) == 1) and np.all(y.sum(-1) == 1)):
        raise ValueError("targets must be one-hot rows%s (as the reference's data_generator yields) or int ids of rank %d"
                         % ("" if vocab is None else " of width %d" % vocab, ids_rank))
    return y.argmax(-1).astype(np.int32)


class KerasLikeModel(object):
    """Sub-classes provide: self.store (ParamStore), self.device, _init_runtime() in their constructor, _forward_train(), _backward(), what
    train_step asks about a batch (_step_key, _stage_batch), the *_on_batch_device forms and predict().
    _backward() announces finished layer ranges to self.grad_sync.ready (when the exchange has one); nothing per-step is stored on the model for it."""

    optimizer = None
    loss = None
    MAX_STEP_GRAPHS = 4        # batch shapes kept as captured graphs; further shapes run eagerly
    use_step_graph = True      # (one GPU) replay the train step from a hipGraph; DCAP_STEP_GRAPH=0 overrides

    def _init_runtime(self):
        """What a step keeps on the model beside its weights."""
        self.grad_sync = None                     # set by ParallelModel: called between backward and the update
        self._bufs = {}                           # scratch buffers by name (_buf)
        self._steps = {}                          # captured train steps by batch shape (step_graph.CapturedStep)

    def compile(self, optimizer, loss=None):
        """optimizer: a params.Adam / params.SGD instance, or "adam" / "sgd" (Keras' defaults)."""
        self.optimizer, self.loss = (get_optimizer(optimizer) if isinstance(optimizer, str) else optimizer), loss
        self._invalidate_graphs()              # captured train steps hold the previous optimizer's state tensors

    def _invalidate_graphs(self):
        """Drop the captured train steps (step_graph.CapturedStep per batch shape): something they baked has moved."""
        self._steps = step_graph.drop_all(getattr(self, "_steps", {}))      # (first called while the model is built)

    # ---- the train step: eager, or through the captured step of its batch shape ------------------------------------------
    def _buf(self, key, shape, dtype=torch.float32):
        b = self._bufs.get(key)
        if b is None or tuple(b.shape) != tuple(shape) or b.dtype != dtype:
            b = torch.empty(shape, dtype=dtype, device=self.device)
            self._bufs[key] = b
        return b

    def _dev_feat(self, feat):
        if isinstance(feat, torch.Tensor):
            return feat.to(self.device, torch.float32).contiguous()
        return torch.tensor(np.ascontiguousarray(feat, np.float32), device=self.device)

    def _captured_step(self, key, feat):
        """-> (the CapturedStep this batch runs through, is it new) or (None, False): the step runs eagerly -- a gradient exchange is
        attached (its collectives are issued from Python; a hook without `.world` counts as one), graphs are switched off, or
        MAX_STEP_GRAPHS other shapes are held already.  cs.feat: the persistent device tensor the caller copies the features into."""
        world = 1 if self.grad_sync is None else getattr(self.grad_sync, "world", None)
        cs = self._steps.get(key)
        if world != 1 or not self.use_step_graph or not step_graph.enabled() or (cs is None and len(self._steps) >= self.MAX_STEP_GRAPHS):
            return None, False
        new = cs is None
        if new:
            cs = self._steps[key] = step_graph.CapturedStep()
            cs.feat = torch.empty(tuple(feat.shape), dtype=torch.float32, device=self.device)
        return cs, new

    def _run_captured(self, cs, body, counters_get, counters_set, on_replay):
        own, self._bufs = self._bufs, cs.bufs                # this shape's private scratch buffers (see CapturedStep)
        try:
            return cs.run(body, counters_get, counters_set, on_replay)
        finally:
            self._bufs = own

    def _grads_ready(self, *layers):
        """Data parallel: these layers' gradients are final -- start their all-reduce while the backward goes on."""
        if self.grad_sync is not None and hasattr(self.grad_sync, 'ready'):
            for layer in layers:
                lo, hi = self.store.layer_range(layer)
                self.grad_sync.ready(self.store.flat_grad, lo, hi)

    def _step_loss(self, loss_rows, *batch):
        """The step's loss tensor from the forward pass's loss rows (batch: the step's, for a sub-class that reports more than the loss)."""
        return ops.mean(loss_rows, out=self._buf('loss', (1,)))

    def _step_launches(self, *batch, lr_t_dev=None, **forward_kw):
        """THE train step, launch by launch: forward (batch, forward_kw: what the sub-class's _forward_train takes), loss, backward,
        (all-reduce), the optimizer's launch.  Issued as it stands (lr_t_dev None: the update's step word is a launch argument and an
        attached gradient exchange runs between backward and update) and as the body of a captured step (lr_t_dev: the device word the
        replayed update reads it from; a step with an exchange attached is never captured, _captured_step)."""
        loss_rows, _ = self._forward_train(*batch, want_grad=True, **forward_kw)
        loss = self._step_loss(loss_rows, *batch)
        self._backward()
        scale = self.grad_sync(self.store.flat_grad) if lr_t_dev is None and self.grad_sync is not None else 1.0
        self.optimizer.apply(self.store, grad_scale=scale, lr_t_dev=lr_t_dev)
        return loss

    def _train_step_eager(self, *batch):
        return self._step_launches(*batch)

    # What a sub-class says about its step: _step_key, _stage_batch and, with host counters of its own, the three _counters hooks.
    def _step_key(self, *batch):
        """What the captured launches bake of this batch, the feature shape first; None: this batch never replays."""
        raise NotImplementedError

    def _stage_batch(self, cs, new, *batch):
        """Bring the batch into cs's persistent buffers (new: make them first) -> (the staged batch, forward_kw, the device lr_t word)."""
        raise NotImplementedError

    def _stage_lr_t(self, cs, new):
        """The step word of the coming update as a one-word upload of its own -> its device view (for batches that are on the device already)."""
        if new:
            cs.scalars = step_graph.PackedInputs(self.device, [("lr_t", 1)])
        cs.scalars.upload({"lr_t": step_graph.lr_word(self.optimizer)})
        return cs.scalars.view("lr_t", torch.float32)

    def _counters(self):
        """The host-side counters a step advances (restored when a capture fails: the eager retry advances them again)."""
        return self.optimizer.iterations

    def _set_counters(self, v):
        self.optimizer.iterations = v

    def _advance_counters(self, cs):
        """What the captured Python did once, by hand after every replay of cs."""
        self.optimizer.iterations += 1

    def train_step(self, *batch):
        """forward + loss + backward + (all-reduce) + the optimizer's update on what the sub-class's _forward_train takes; the loss terms
        as a DEVICE tensor (no sync).  With use_step_graph (one GPU; DCAP_STEP_GRAPH=0 overrides) the step is replayed from a hipGraph
        captured on the third call with a batch shape (step_graph.py): the batch reaches it through the shape's persistent buffers."""
        if self.optimizer is None:
            raise RuntimeError("compile(optimizer, loss) first")
        key = self._step_key(*batch)
        cs, new = (None, False) if key is None else self._captured_step(tuple(key) + (self.optimizer.baked_key(),), batch[0])
        if cs is None:
            return self._step_launches(*batch)
        staged, forward_kw, lr_t_dev = self._stage_batch(cs, new, *batch)
        return self._run_captured(cs, lambda: self._step_launches(*staged, lr_t_dev=lr_t_dev, **forward_kw), self._counters, self._set_counters,
                                  lambda: self._advance_counters(cs))

    @property
    def trainable_weights(self):
        return list(self.store.trainable_names)

    @property
    def non_trainable_weights(self):
        return list(self.store.frozen_names)

    def get_weights_dict(self):
        return self.store.to_numpy()

    def save_weights(self, path):
        save_weight_file(path, self.get_weights_dict())

    def _stored_shape(self, name):
        """The shape `name` has in a weight file (a sub-class that holds a weight in another layout than Keras': with _to_held)."""
        return tuple(self.store.w[name].shape)

    def _to_held(self, name, array):
        """A stored array in the layout the model holds it in."""
        return array

    def load_weights(self, filepath, by_name=False, skip_mismatch=False):
        loaded = load_weight_file(filepath) if isinstance(filepath, str) else dict(filepath)
        for k, v in loaded.items():
            if k not in self.store.w:
                if by_name:
                    continue
                raise KeyError("weight %s is not part of this model" % k)
            if tuple(np.shape(v)) != self._stored_shape(k):
                if skip_mismatch:
                    continue
                raise ValueError("shape mismatch for %s: %s vs %s" % (k, tuple(np.shape(v)), self._stored_shape(k)))
            self.store.assign(k, self._to_held(k, v), refresh=False)
        self._weights_changed()

    def _weights_changed(self):
        """Master weights were rewritten from outside the optimizer (load_weights, ParallelModel's broadcast): re-cast the bf16
        operand copies the bf16 GEMMs read (compute_dtype='bf16'); sub-classes also re-derive what they fold from weights."""
        self._invalidate_graphs()
        self.store.refresh_shadow()

    def summary(self):
        lines = ["%-40s %-22s %s" % ("weight", "shape", "trainable")]
        total = train = 0
        for names, tr in ((self.store.trainable_names, True), (self.store.frozen_names, False)):
            for n in names:
                shp = tuple(self.store.w[n].shape)
                k = int(np.prod(shp))
                total += k
                train += k if tr else 0
                lines.append("%-40s %-22s %s" % (n, shp, tr))
        lines.append("Total params: %d  Trainable: %d  Non-trainable: %d" % (total, train, total - train))
        return "\n".join(lines)

    # ---- losses without a host round trip --------------------------------------------------------------------------------
    # train_on_batch / test_on_batch return Python floats like Keras and therefore wait for the step.  Training loops
    # (fit_generator, ParallelModel) use the *_device forms instead: a float32 DEVICE tensor of the step's loss terms, nothing
    # synchronised; _losses_to_api turns its host copy into what the Keras call returns.
    def train_on_batch_device(self, inputs, targets):
        raise NotImplementedError

    def test_on_batch_device(self, inputs, targets):
        raise NotImplementedError

    @staticmethod
    def _losses_to_api(v):
        return float(v[0])

    def train_on_batch(self, inputs, targets):
        """keras.Model.train_on_batch: the loss (a model with metrics: [loss, metrics...]) as Python floats."""
        return self._losses_to_api(self.train_on_batch_device(inputs, targets).cpu().numpy())

    def test_on_batch(self, inputs, targets):
        return self._losses_to_api(self.test_on_batch_device(inputs, targets).cpu().numpy())

    def fit_generator(self, generator, epochs=1, steps_per_epoch=None, callbacks=None, validation_data=None,
                      verbose=1, max_queue_size=10, workers=1, use_multiprocessing=False, initial_epoch=0):
        """keras.Model.fit_generator as the reference calls it (text_generation_model_v2.py:300-313: workers=1,
        max_queue_size=10; text_generation_model.py:458-472: max_queue_size=100).  Keras' GeneratorEnqueuer semantics:
        workers >= 1 runs next(generator) on ONE background thread per worker filling a queue of at most max_queue_size batches
        (threads, not processes: use_multiprocessing=True with a plain generator is refused like Keras warns against; more than
        one worker needs a thread-safe generator exactly as in Keras); workers=0 runs the generator on the calling thread.
        The loop itself never waits for the GPU: step losses stay on the device and are read once per epoch."""
        if use_multiprocessing:
            raise NotImplementedError("use_multiprocessing=True duplicates a plain generator in every process (Keras warns about it); "
                                      "the reference uses threads (use_multiprocessing=False)")
        if steps_per_epoch is None:
            raise ValueError("steps_per_epoch is required for a generator")
        outer = getattr(self, "_outer", None) or self          # under ParallelModel the loop feeds GLOBAL batches through the wrapper
        enq = GeneratorEnqueuer(generator, workers, max_queue_size) if workers and workers > 0 else None
        batches = enq.get() if enq is not None else generator
        history = []
        try:
            for epoch in range(initial_epoch, epochs):
                acc = None
                for _ in range(steps_per_epoch):
                    inputs, targets = next(batches)
                    step = outer.train_on_batch_device(inputs, targets)      # device tensor; its buffer is reused by the next step
                    acc = step.clone() if acc is None else acc.add_(step)    # (bookkeeping on the step's stream, not model arithmetic)
                logs = {"loss": float((acc / steps_per_epoch).cpu().numpy()[0])}       # the epoch's ONE host sync (a model's metrics come after the loss)
                if validation_data is not None:
                    logs["val_loss"] = float(outer.test_on_batch(validation_data[0], validation_data[1]))
                if verbose and getattr(self, "is_chief", True):
                    print("Epoch %d/%d - " % (epoch + 1, epochs) + " - ".join("%s: %.4f" % kv for kv in sorted(logs.items())))
                if getattr(self, "is_chief", True):
                    for cb in callbacks or []:
                        cb.on_epoch_end(self, epoch, logs)
                history.append(logs)
        finally:
            if enq is not None:
                enq.stop()
        return history


class GeneratorEnqueuer(object):
    """keras.utils.GeneratorEnqueuer(generator, use_multiprocessing=False): `workers` daemon threads call next(generator)
    (under a lock: a Python generator is not re-entrant; with one worker -- the reference's setting -- the lock is free) and put
    batches into a bounded queue; get() yields them in arrival order.  A generator that raises ends the stream with that error;
    StopIteration ends it cleanly."""

    _END = object()

    def __init__(self, generator, workers=1, max_queue_size=10):
        import queue
        import threading
        self._gen, self._q = generator, queue.Queue(maxsize=max(1, int(max_queue_size)))
        self._stop, self._lock = threading.Event(), threading.Lock()
        self._threads = [threading.Thread(target=self._work, daemon=True) for _ in range(max(1, int(workers)))]
        for t in self._threads:
            t.start()

    def _put(self, item):
        import queue
        while not self._stop.is_set():
            try:
                self._q.put(item, timeout=0.05)
                return
            except queue.Full:
                continue

    def _work(self):
        while not self._stop.is_set():
            try:
                with self._lock:
                    item = next(self._gen)
            except StopIteration:
                self._put(self._END)
                return
            except BaseException as e:          # hand the error to the consumer
                self._put(e)
                return
            self._put(item)

    def get(self):
        while True:
            item = self._q.get()
            if item is self._END:
                return
            if isinstance(item, BaseException):
                raise item
            yield item

    def stop(self):
        self._stop.set()
        for t in self._threads:
            t.join(timeout=5)
