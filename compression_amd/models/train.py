"""Training of the image models: what `model.compile(...)` + `model.fit(...)` do in the model scripts
(models/bls2017.py:124-162, 235-270), for any module whose `forward(x, training)` returns `(loss, bpp, mse)`.

    train_step / test_step    bls2017.py:124-140
    loss, bpp, mse metrics    tf.keras.metrics.Mean: running sums kept on the device, read once per epoch
    TerminateOnNaN            a sticky device flag; the optimiser launch of the bad batch and of every later one is
                              skipped on the device (`KerasAdam.step(skip=)`), the flag is read every `nan_check_every` steps
    BackupAndRestore          `train_path/backup.pt` after every epoch, removed when training completes
    TensorBoard               one JSON line per epoch in `train_path/metrics.jsonl`
    fit() ends with           `model.init_compression()` (bls2017.py:157-162)"""
from __future__ import annotations

import inspect
import json
import math
import os

import torch

from ..optimizers import KerasAdam

__all__ = ["Trainer"]

METRICS = ("loss", "bpp", "mse")


class Trainer:
    def __init__(self, model, optimizer=None, train_path=None, nan_check_every=100):
        self.model = model
        self.optimizer = optimizer          # None: KerasAdam(lr=1e-4), created in front of the first step (`build`)
        self.train_path = None if train_path is None else os.fspath(train_path)
        self.nan_check_every = int(nan_check_every)
        self.stop_message = None
        self._built = False
        self.device = next(model.parameters()).device
        self._sums = torch.zeros(len(METRICS), dtype=torch.float64, device=self.device)
        self._count = 0
        self._nan_flag = torch.zeros(1, dtype=torch.int32, device=self.device)        # sticky
        self._nan_batch = torch.full((1,), -1, dtype=torch.int64, device=self.device)  # the first bad batch of its epoch
        self._batch = 0

    # ---------------------------------------------------------------------------------------------------------------

    def reset_metrics(self):
        self._sums.zero_()
        self._count = 0

    def _update_metrics(self, values):
        self._sums += torch.stack([v.detach().to(torch.float64) for v in values])
        self._count += 1

    def result(self, prefix=""):
        """The means since `reset_metrics()`; one read of the device."""
        sums = self._sums.tolist()
        return {prefix + name: (s / self._count if self._count else float("nan")) for name, s in zip(METRICS, sums)}

    def build(self, x):
        """The models' GDN layers create their parameters on the first call: one forward pass without gradients (no
        noise is drawn with training=False) makes `model.parameters()` complete, then the default optimiser is
        created over them.  An optimiser passed to the constructor must already hold every parameter."""
        if self.optimizer is None:
            with torch.no_grad():
                self.model(x, training=False)
            self.optimizer = KerasAdam(self.model.parameters(), lr=1e-4)
        self._takes_skip = "skip" in inspect.signature(self.optimizer.step).parameters
        self._built = True

    def train_step(self, x):
        """zero_grad, forward, backward, optimiser step -> (loss, bpp, mse) as device scalars.  Nothing waits for the
        device, unless the optimiser has no `skip` argument: then the flag is read in front of its step."""
        if not self._built:
            self.build(x)
        self.optimizer.zero_grad()
        loss, bpp, mse = self.model(x, training=True)
        loss.backward()
        bad = ~torch.isfinite(loss.detach()).reshape(1)
        first = bad & (self._nan_flag == 0)
        self._nan_batch.copy_(torch.where(first, torch.full_like(self._nan_batch, self._batch), self._nan_batch))
        self._nan_flag |= bad.to(torch.int32)
        if self._takes_skip:
            self.optimizer.step(skip=self._nan_flag)
        elif int(self._nan_flag) == 0:
            self.optimizer.step()
        self._update_metrics((loss, bpp, mse))
        self._batch += 1
        return loss.detach(), bpp.detach(), mse.detach()

    @torch.no_grad()
    def test_step(self, x):
        loss, bpp, mse = self.model(x, training=False)
        self._update_metrics((loss, bpp, mse))
        return loss, bpp, mse

    def _terminated(self):
        """Reads the flag (one device read); True once a loss was not finite."""
        if int(self._nan_flag) == 0:
            return False
        if self.stop_message is None:
            self.stop_message = f"Batch {int(self._nan_batch)}: Invalid loss, terminating training"
            print(self.stop_message)
        return True

    # ---------------------------------------------------------------------------------------------------------------
    # backup

    def _backup_file(self):
        return os.path.join(self.train_path, "backup.pt")

    def _rng_state(self):
        state = {"cpu": torch.get_rng_state()}
        if self.device.type == "cuda":
            state["device"] = torch.cuda.get_rng_state(self.device)
        return state

    def _save_backup(self, dataset, epoch, history):
        state = {"model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(),
                 "dataset": dataset.state_dict() if hasattr(dataset, "state_dict") else None,
                 "epoch": epoch, "history": history, "rng": self._rng_state()}
        tmp = self._backup_file() + ".tmp"
        torch.save(state, tmp)
        os.replace(tmp, self._backup_file())

    def _restore_backup(self, dataset):
        """-> (the number of epochs done, their history), from the backup if there is one."""
        if self.train_path is None or not os.path.exists(self._backup_file()):
            return 0, []
        state = torch.load(self._backup_file(), map_location="cpu", weights_only=False)
        self.model.load_state_dict(state["model"])
        self.optimizer.load_state_dict(state["optimizer"])
        if state["dataset"] is not None:
            dataset.load_state_dict(state["dataset"])
        torch.set_rng_state(state["rng"]["cpu"])
        if "device" in state["rng"] and self.device.type == "cuda":
            torch.cuda.set_rng_state(state["rng"]["device"], self.device)
        return state["epoch"], list(state["history"])

    # ---------------------------------------------------------------------------------------------------------------

    def fit(self, train_dataset, epochs, steps_per_epoch, validation_data=None, verbose=False):
        """Trains up to `epochs` epochs of `steps_per_epoch` batches of `train_dataset` (continuing from the backup in
        `train_path` if there is one) and returns the history: one dict of loss, bpp, mse (and val_*) per epoch.
        `validation_data` is materialised once and reused every epoch.  Ends with `model.init_compression()`."""
        if self.train_path is not None:
            os.makedirs(self.train_path, exist_ok=True)
        validation = None if validation_data is None else list(validation_data)
        self._nan_flag.zero_()              # sticky within one fit(), not across two
        self.stop_message = None
        batches = iter(train_dataset)
        pending = []
        if not self._built:
            pending.append(next(batches))           # the first batch also builds the lazily created parameters
            self.build(pending[0])
        first_epoch, history = self._restore_backup(train_dataset)
        if first_epoch:
            pending, batches = [], iter(train_dataset)      # the dataset is back where the backup was taken
        for epoch in range(first_epoch, epochs):
            self.model.train()
            self.reset_metrics()
            self._batch = 0
            stop = False
            for step in range(steps_per_epoch):
                try:
                    x = pending.pop() if pending else next(batches)
                except StopIteration:
                    break
                self.train_step(x)
                if (step + 1) % self.nan_check_every == 0 and self._terminated():
                    stop = True
                    break
            stop = stop or self._terminated()
            logs = self.result()
            if validation and not stop:
                self.reset_metrics()
                for x in validation:
                    self.test_step(x)
                logs.update(self.result("val_"))
            history.append(logs)
            if verbose:
                print(f"Epoch {epoch + 1}/{epochs}: " + " - ".join(f"{k}: {v:.4f}" for k, v in logs.items()))
            if self.train_path is not None:
                with open(os.path.join(self.train_path, "metrics.jsonl"), "a") as f:
                    # a mean that is not finite (the epoch TerminateOnNaN ends) is written as null: NaN is not JSON
                    finite = {k: (v if math.isfinite(v) else None) for k, v in logs.items()}
                    f.write(json.dumps({"epoch": epoch + 1, **finite}, allow_nan=False) + "\n")
            if stop:
                break
            if self.train_path is not None:
                self._save_backup(train_dataset, epoch + 1, history)
        if self.train_path is not None and os.path.exists(self._backup_file()):
            os.remove(self._backup_file())
        self.model.init_compression()
        return history
