"""The reference's training driver (``train.py:330-617``, and the identical loop of ``kd_train.py``) around the HIP
training step: tuple sampling, hard-negative mining against cached descriptors, periodic evaluation loss, cache refresh
and checkpointing -- the control flow and its constants restated, the compute on the GPU:

  * one step                    train.py:484-495   -> ``TrainStep.step`` / ``DistillStep.step``
  * descriptor of one cloud     train.py:820-855   -> the fused inference pipeline with the CURRENT weights
  * cached descriptors          train.py:871-965   -> ``retrieval.get_latent_vectors`` (row i = training cloud i)
  * hard negatives              train.py:857-869   -> exact GPU k-NN over the 4000 sampled negatives' cached descriptors
                                                      (sklearn KDTree in the reference)
  * the same three by record id train.py:820-965   -> ``Trainer(bank=True, device_mining=True)``: ``engine.forward_bank``,
                                                      ``retrieval.latent_vectors_bank`` and ``retrieval.mine_topk`` on the cloud bank
  * checkpoints                 train.py:611-617   -> TensorFlow bundle files (``tf_bundle.write_checkpoint``), same
                                                      variable names, readable by ``tf.train.Saver`` and by this package

The host side stays numpy / random exactly like the reference (``random.shuffle`` of the positive / negative lists,
``np.random.shuffle`` of the epoch order), so a seeded run visits the same tuples."""
from __future__ import annotations

import logging
import os
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from . import tf_bundle
from . import lib as L
from .retrieval import get_latent_vectors, latent_vectors_bank
from .utils.loading_pointclouds import NUM_POINTS, get_query_tuple, get_query_tuple_ids, get_random_hard_negatives
from .variables import variable_scope

SAMPLED_NEG = 4000     # train.py:340
NUM_TO_TAKE = 10       # train.py:343
EVAL_BATCHES = 5       # train.py:527


class Trainer:
    def __init__(self, step, train_queries: Optional[Dict[int, dict]], train_data: np.ndarray,
                 test_queries: Optional[Dict[int, dict]] = None, test_data: Optional[np.ndarray] = None,
                 save_path: Optional[str] = None, logger: Optional[logging.Logger] = None, graph: bool = False,
                 bank: bool = False, device_mining: bool = False, poses=None, tuple_seed: int = 0, r_pos: float = 10.0,
                 r_neg: float = 50.0):
        """``step``: a TrainStep / DistillStep; ``*_queries``: the pickles of generate_training_tuples (key -> {'query',
        'positives', 'negatives'}); ``*_data``: (T, 4096, INPUT_DIM) float32 arrays in key order (train.py:159-190).
        ``bank=True``: ``train_data`` is uploaded ONCE into an ``ops.CloudBank`` (sorted clouds + finished kNN graphs, ~0.65 MB per
        4096-point cloud of device memory) and the loop steps on cloud ids (``step.step_ids``): no per-step tuple assembly and
        upload on the host, no per-step sort / kNN / transposition on the device; same tuples, same losses, bit for bit.  It serves
        the unaugmented protocol of train.py:388.  ``evaluate_loss``, the mining and the descriptor cache keep reading the arrays
        unless ``device_mining=True`` (needs the bank): the query's descriptor and the refreshed descriptor cache then come from the
        bank's records by id (``engine.forward_bank``) and stay on the device, and the hard negatives of a key are searched there
        (``retrieval.mine_topk``) -- per key one upload of the sampled ids and one copy of the NUM_TO_TAKE mined ids back; the
        shuffles and the tuple logic stay on the host, so a seeded run mines the same negatives and steps alike, bit for bit.
        ``poses`` ((T, 2) float64 northing / easting of the records, numpy or torch; needs ``bank=True, device_mining=True``): the
        tuples are drawn on the device from the poses (``ops.PoseTuples``: positives within ``r_pos``, negatives beyond ``r_neg``, the
        reference's other-negative rule) and ``train_queries`` may be None -- no pickle, no Python lists.  Per iteration: candidates ->
        ``forward_bank`` -> ``mine_topk`` (both only once a descriptor cache exists) -> sample -> ``step_ids``, all on the device; the
        only host read is the loss.  Keys with fewer than P positives leave the epoch's permutation up front.  The draw is a fixed hash of
        (``tuple_seed``, global step, key): a NEW sampling stream -- deterministic, but it does not reproduce a seeded run of the host
        path.  ``HARD_NEGATIVES`` is not consulted on this path; ``evaluate_loss`` keeps reading ``test_queries``."""
        if device_mining and not bank:
            raise ValueError("device_mining=True needs bank=True: the mining reads the clouds by record id")
        if poses is not None and not (bank and device_mining):
            raise ValueError("poses= needs bank=True and device_mining=True: the tuples are drawn and mined on the device by record id")
        if poses is None and train_queries is None:
            raise ValueError("train_queries may be None only with poses=")
        self.step = step
        self.params = step.params
        self.TRAINING_QUERIES, self.train_data = train_queries, train_data
        self.TEST_QUERIES, self.test_data = test_queries, test_data
        self.save_path = save_path
        self.graph = graph     # replay the step as one HIP graph (TrainStep.step(graph=True)): every tuple has the same shape
        self.log = logger or logging.getLogger("epcnet.train")
        self.HARD_NEGATIVES: Dict[int, List[int]] = {}      # train.py:97 (never filled by the reference either)
        self.TRAINING_LATENT_VECTORS = []                   # train.py:98
        p = self.params
        self.B = int(p.get("BATCH_NUM_QUERIES", 1))
        self.P = int(p.get("POSITIVES_PER_QUERY", p.get("TRAIN_POSITIVES_PER_QUERY", 2)))
        self.N = int(p.get("NEGATIVES_PER_QUERY", p.get("TRAIN_NEGATIVES_PER_QUERY", 14)))
        self.max_epoch = int(p.get("MAX_EPOCH", 20))
        self.num_points = int(p.get("NUM_POINTS", NUM_POINTS))
        self.device = step.store.device
        self.history: List[dict] = []
        self.bank = self._build_bank(train_data) if bank else None
        self.device_mining = bool(device_mining)
        self._table_src, self._table_dev = None, None       # the caller's numpy descriptor cache and its device copy (by identity)
        self._mine_host, self._mine_dev, self._mine_ws = None, None, None
        self.tuples, self._enough, self._cand = None, None, None
        if poses is not None:
            from . import ops
            self.tuples = ops.PoseTuples(poses, r_pos=r_pos, r_neg=r_neg, seed=tuple_seed, device=self.device)
            if len(self.tuples) != int(train_data.shape[0]):
                raise ValueError("poses has %d rows for %d training clouds" % (len(self.tuples), int(train_data.shape[0])))

    def _build_bank(self, data: np.ndarray):
        """Upload ``data`` (T, n, 3) into a CloudBank, in slices that bound the staging copy; logs the one-time cost."""
        import time
        from . import ops
        t0 = time.perf_counter()
        bank = ops.CloudBank(int(data.shape[1]), int(data.shape[0]), self.device)
        for a in range(0, int(data.shape[0]), 1024):
            bank.add(torch.as_tensor(data[a:a + 1024], dtype=torch.float32).to(self.device))
        torch.cuda.synchronize(self.device)
        self.log.info("Cloud bank: %d clouds, %.1f MB on %s (%d bytes per cloud), built in %.2f s", len(bank),
                      len(bank) * bank.bytes_per_cloud / 1e6, self.device, bank.bytes_per_cloud, time.perf_counter() - t0)
        return bank

    # ---- inference with the current weights ------------------------------------------------------------------------
    def _engine(self):
        with variable_scope(self.step.outer):
            scope = getattr(self.step.model, "BACKBONE_SCOPE", "fastdgcnn")
            return self.step.model.engine_for(self.step.model.ARCH, self.params, backbone_scope=scope)

    def get_feature_representation(self, idx: int) -> np.ndarray:
        """train.py:820-855: the descriptor of training cloud ``idx`` (is_training=False)."""
        self.step._ensure_built(int(self.train_data.shape[1]))
        return get_latent_vectors(self._engine(), self.train_data[[idx]], batch_size=1, device=self.device)[0]

    def get_latent_vectors(self, data: Optional[np.ndarray] = None) -> np.ndarray:
        """train.py:871-965: descriptors of every training cloud, row i = cloud i."""
        self.step._ensure_built(int(self.train_data.shape[1]))
        return get_latent_vectors(self._engine(), self.train_data if data is None else data, batch_size=64,
                                  device=self.device)

    # ---- tuples ---------------------------------------------------------------------------------------------------------
    def _tuples(self, keys, queries, data, hard_negs_of: Optional[Callable[[int], List[int]]]):
        """The per-batch tuple assembly of train.py:356-425 / :535-561.  Returns (arrays or None, reason)."""
        tuples = []
        for key in keys:
            if len(queries[key]["positives"]) < self.P:
                return None, "FAULTY TUPLE"
            hard = hard_negs_of(key) if hard_negs_of is not None else []
            tuples.append(get_query_tuple(key, queries[key], self.P, self.N, queries, hard_neg=hard, other_neg=True,
                                          data=data))
            if tuples[-1][3].shape[0] != self.num_points:                                       # train.py:401
                return None, "NO OTHER NEG"
        q = np.expand_dims(np.array([t[0] for t in tuples]), axis=1)
        o = np.expand_dims(np.array([t[3] for t in tuples]), axis=1)
        pos = np.array([t[1] for t in tuples])
        neg = np.array([t[2] for t in tuples])
        if q.ndim != 4:
            return None, "FAULTY TUPLE"
        dev = lambda a: torch.as_tensor(a, dtype=torch.float32).to(self.device)
        return (dev(q), dev(pos), dev(neg), dev(o)), ""

    def _tuple_ids(self, keys, queries, hard_negs_of: Optional[Callable[[int], List[int]]]):
        """``_tuples`` for the cloud bank: the same draws (``random`` consumed identically) and the same skips, as id arrays
        (B,1), (B,P), (B,Nn), (B,1) for ``step.step_ids``.  Returns (arrays or None, reason)."""
        tuples = []
        for key in keys:
            if len(queries[key]["positives"]) < self.P:
                return None, "FAULTY TUPLE"
            hard = hard_negs_of(key) if hard_negs_of is not None else []
            tuples.append(get_query_tuple_ids(int(key), queries[key], self.P, self.N, queries, hard_neg=hard, other_neg=True))
            if len(tuples[-1][3]) != 1:                                                          # train.py:401
                return None, "NO OTHER NEG"
        as_ids = lambda rows: np.asarray(rows, dtype=np.int64).reshape(len(tuples), -1)
        return (as_ids([[t[0]] for t in tuples]), as_ids([t[1] for t in tuples]), as_ids([t[2] for t in tuples]),
                as_ids([t[3] for t in tuples])), ""

    def _mining_table(self) -> torch.Tensor:
        """The descriptor cache as a device tensor: what the refresh left, or the caller's numpy array uploaded once."""
        t = self.TRAINING_LATENT_VECTORS
        if torch.is_tensor(t) and t.is_cuda:
            return t
        if self._table_src is not t:
            self._table_dev = torch.as_tensor(np.asarray(t), dtype=torch.float32).to(self.device).contiguous()
            self._table_src = t
        return self._table_dev

    def _mine_on_device(self, key: int, negatives: List[int]) -> List[int]:
        """train.py:820-855 + :857-869 on the bank: descriptor of record ``key`` -> its NUM_TO_TAKE nearest among the cached descriptors
        of ``negatives``.  One int32 buffer {key, count, ids ...} goes up, the mined ids come back."""
        from .retrieval import mine_topk
        table = self._mining_table()
        if self._mine_dev is None:
            self._mine_host = torch.zeros(2 + SAMPLED_NEG, dtype=torch.int32).pin_memory()
            self._mine_dev = torch.zeros(2 + SAMPLED_NEG, dtype=torch.int32, device=self.device)
            self._mine_ws = torch.empty(int(L.lib().epc_mine_topk_workspace_bytes(1, SAMPLED_NEG)), dtype=torch.uint8,
                                        device=self.device)
        m = len(negatives)
        host = self._mine_host.numpy()           # (the previous key's copy has completed: its result was read back)
        host[0], host[1] = int(key), m
        host[2:2 + m] = np.asarray(negatives, dtype=np.int32)
        self._mine_dev[:2 + m].copy_(self._mine_host[:2 + m], non_blocking=True)
        self.step._ensure_built(self.bank.n)
        query = self._engine().forward_bank(self.bank, self._mine_dev[0:1])
        k = min(NUM_TO_TAKE, m)                  # (retrieval.knn_search: k = min(k, rows))
        _, _, ids = mine_topk(table, query, self._mine_dev[2:].view(1, SAMPLED_NEG), self._mine_dev[1:2], k, workspace=self._mine_ws)
        # (a slot without a neighbour at a finite distance indexes the list with -1 on the host path: its last entry)
        return [int(v) if v >= 0 else int(negatives[-1]) for v in ids[0].cpu().tolist()]

    def _tuple_ids_from_poses(self, keys: torch.Tensor):
        """The id tensors of ``step.step_ids`` for ``keys`` ((B,) int32 on the device), drawn there: candidates -> descriptor of the key
        -> mined hard negatives (once a descriptor cache exists: train.py:373-377 / :390-395) -> sample.  Four launches plus the
        inference pass; nothing is read back."""
        from .retrieval import mine_topk
        step, hard = int(self.step.global_step), None
        if len(self.TRAINING_LATENT_VECTORS) != 0:
            B = int(keys.numel())
            if self._cand is None or int(self._cand[0].shape[0]) != B:
                self._cand = (torch.empty((B, SAMPLED_NEG), dtype=torch.int32, device=self.device),
                              torch.empty(B, dtype=torch.int32, device=self.device),
                              torch.empty(int(L.lib().epc_mine_topk_workspace_bytes(B, SAMPLED_NEG)), dtype=torch.uint8, device=self.device))
            cand, count = self.tuples.candidates(keys, step, SAMPLED_NEG, out=self._cand[:2])
            self.step._ensure_built(self.bank.n)
            query = self._engine().forward_bank(self.bank, keys)
            _, _, hard = mine_topk(self._mining_table(), query, cand, count, NUM_TO_TAKE, workspace=self._cand[2])
        ids, _ = self.tuples.sample(keys, step, self.P, self.N, hard=hard)
        return ids[:, :1], ids[:, 1:1 + self.P], ids[:, 1 + self.P:1 + self.P + self.N], ids[:, 1 + self.P + self.N:]

    def _hard_negatives(self, key: int) -> List[int]:
        """train.py:373-377 / :390-395 (the three cache states)."""
        if len(self.TRAINING_LATENT_VECTORS) == 0:
            return []
        if self.device_mining:
            np.random.shuffle(self.TRAINING_QUERIES[key]["negatives"])
            hard = self._mine_on_device(int(key), self.TRAINING_QUERIES[key]["negatives"][0:SAMPLED_NEG])
        else:
            query = self.get_feature_representation(key)
            np.random.shuffle(self.TRAINING_QUERIES[key]["negatives"])
            negatives = self.TRAINING_QUERIES[key]["negatives"][0:SAMPLED_NEG]
            hard = get_random_hard_negatives(query, negatives, NUM_TO_TAKE, self.TRAINING_LATENT_VECTORS)
        if len(self.HARD_NEGATIVES.keys()) != 0:
            hard = list(set().union(self.HARD_NEGATIVES[key], hard))
        return hard

    # ---- one epoch -------------------------------------------------------------------------------------------------------
    def train_one_epoch(self, epoch: int, max_iters: Optional[int] = None) -> List[float]:
        """train.py:330-617.  ``max_iters`` truncates the epoch (tests / smoke runs); None = the whole epoch."""
        from . import distributed as D
        rank, world = D.world()
        idxs = np.arange(0, len(self.tuples) if self.tuples is not None else len(self.TRAINING_QUERIES.keys()))
        np.random.shuffle(idxs)
        if world > 1:
            # data-parallel over tuples: every rank must walk the SAME permutation (rank 0's) and take its own
            # slice of every global batch of world * B queries; the ranks step -- or skip -- together
            perm = torch.as_tensor(idxs, dtype=torch.int64, device=self.device)
            D.broadcast_tensors([perm], src=0)
            idxs = perm.cpu().numpy()
        perm_dev = None
        if self.tuples is not None:
            # the reference's "FAULTY TUPLE" (fewer than P positives), decided once from the device-side counts instead of per step
            if self._enough is None:
                self._enough = (self.tuples.counts >= self.P).cpu().numpy()
            kept = idxs[self._enough[idxs]]
            self.log.info("Epoch %d: %d of %d keys have fewer than %d positives and are left out", epoch, len(idxs) - len(kept),
                          len(idxs), self.P)
            idxs = kept
            perm_dev = torch.from_numpy(idxs.astype(np.int32)).to(self.device)     # the epoch's keys, uploaded once
        iter_num = len(idxs) // (self.B * world)
        losses = []
        for i in range(iter_num if max_iters is None else min(iter_num, max_iters)):
            base = (i * world + rank) * self.B
            keys = idxs[base:base + self.B]
            if perm_dev is not None:
                batch, why = self._tuple_ids_from_poses(perm_dev[base:base + self.B]), ""
            elif self.bank is not None:
                batch, why = self._tuple_ids(keys, self.TRAINING_QUERIES, self._hard_negatives)
            else:
                batch, why = self._tuples(keys, self.TRAINING_QUERIES, self.train_data, self._hard_negatives)
            if perm_dev is None and not D.all_true(batch is not None, self.device):
                # a rank that skipped alone would leave the others waiting in the gradient all-reduce
                self.log.info("Epoch: [%d/%d][%d/%d] %s!!!", epoch, self.max_epoch, i + 1, iter_num,
                              why or "another rank drew a faulty tuple")
                continue
            if self.bank is not None:
                loss, lr, _ = self.step.step_ids(self.bank, *batch, epoch=epoch, graph=self.graph)
            else:
                loss, lr, _ = self.step.step(*batch, epoch=epoch, graph=self.graph) if self.graph else self.step.step(*batch, epoch=epoch)
            losses.append(float(loss))
            if not np.isfinite(losses[-1]) and self.tuples is not None:
                self.tuples.check()     # a slot the draw could not fill (-1: too few negatives, no other negative) raises here, naming the key
            if not np.isfinite(losses[-1]) and self.bank is not None:
                self.bank.check()       # an id outside the bank (a query dict that does not match train_data) raises here, naming the slot
            if not np.isfinite(losses[-1]):
                # A persistent chain launch that was abandoned (a grid barrier ran out of its spin budget) makes the step's returned loss
                # NaN through the verdict the step adds to it (TrainStep._forward_backward; the NaN rows the launch leaves in the concat
                # would not: the ReLUs and hinges drop them).  Say so and reset: this raises EpcNetError.  The step's update has been
                # applied from undefined activations by then -- whoever catches the error goes back to the last checkpoint.
                from . import ops
                ops.chain_persist_check()
            self.history.append({"epoch": epoch, "iter": i, "loss": losses[-1], "lr": lr})
            self.log.info("Epoch: [%d/%d][%d/%d] Loss %.4f lr %.8f", epoch, self.max_epoch, i + 1, iter_num, losses[-1], lr)
            if i % 200 == 7 and self.TEST_QUERIES is not None:                                  # train.py:523-594
                self.log.info("\t\t\teval_loss: %f", self.evaluate_loss(epoch))
            if epoch > 5 and i % (1400 // self.B) == 29:                                        # train.py:597-602
                if self.device_mining:
                    self.step._ensure_built(self.bank.n)
                    self.TRAINING_LATENT_VECTORS = latent_vectors_bank(self._engine(), self.bank)
                else:
                    self.TRAINING_LATENT_VECTORS = self.get_latent_vectors()
                self.log.info("Updated cached feature vectors")
            if i % (6000 // self.B) == 101 and self.save_path and rank == 0:                    # train.py:605-617
                self.log.info("Model saved in file: %s", self.save(epoch, i))     # (the ranks hold identical variables)
        return losses

    def evaluate_loss(self, epoch: int) -> float:
        """train.py:523-594: the loss (is_training=False) averaged over up to 5 random test tuples."""
        idxs = np.arange(0, len(self.TEST_QUERIES.keys()))
        np.random.shuffle(idxs)
        total, counted = 0.0, 0
        for e in range(EVAL_BATCHES):
            keys = idxs[e * self.B:(e + 1) * self.B]
            if len(keys) < self.B:
                break
            batch, _ = self._tuples(keys, self.TEST_QUERIES, self.test_data, None)
            if batch is None:
                continue
            self.step._ensure_built(int(batch[0].shape[2]))
            with torch.no_grad():
                total += float(self.step.compute_loss(*batch, False, None))
            counted += 1
        return total / counted if counted else float("nan")        # (the reference divides by zero here)

    # ---- checkpoints -----------------------------------------------------------------------------------------------------
    def checkpoint_tensors(self) -> Dict[str, np.ndarray]:
        """Everything tf.train.Saver() writes at train.py:611: model variables + step + Adam slots.  The optimizer
        scalars live at the graph root (``Variable``, ``beta1_power``, ``beta2_power``), or under ``student/`` for KD."""
        root = self.step.outer.split("/")[0] + "/" if "/" in self.step.outer else ""
        # plain training: tf.train.Saver() covers the whole graph.  KD: student_saver covers scope `student` only
        # (kd_train.py:525-526) -- no teacher/* variables, and the two beta powers live at the graph root, outside it
        out = {k: v.detach().cpu().numpy() for k, v in self.step.store.state_dict().items() if k.startswith(root)}
        for k, v in self.step.optimizer_state().items():
            if k in ("Variable", "beta1_power", "beta2_power"):
                if root and k != "Variable":
                    continue
                k = root + k
            out[k] = v.detach().cpu().numpy()
        return out

    def save(self, epoch: int, i: int) -> str:
        prefix = os.path.join(self.save_path, "saved_model", "model_epoch%d_iter%d.ckpt" % (epoch, i))   # train.py:612
        os.makedirs(os.path.dirname(prefix), exist_ok=True)
        tf_bundle.write_checkpoint(prefix, self.checkpoint_tensors())
        return prefix

    def restore(self, prefix: str) -> None:
        """train.py:308-315 (RESTORE): model variables, global step and Adam moments."""
        state = tf_bundle.load_checkpoint(prefix)
        self.step._ensure_built(int(self.train_data.shape[1]))
        root_scope = self.step.outer.split("/")[0] + "/" if "/" in self.step.outer else ""
        names = set(k for k in self.step.store.vars.keys() if k.startswith(root_scope))
        missing = sorted(names - set(state.keys()))
        if missing:       # model variables are mandatory (only optimizer slots may be absent: a weights-only checkpoint)
            raise KeyError("checkpoint %s lacks %d model variables, e.g. %s" % (prefix, len(missing), missing[:3]))
        self.step.store.load_state_dict({k: v for k, v in state.items() if k in names}, strict=False)
        root = self.step.outer.split("/")[0] + "/" if "/" in self.step.outer else ""
        opt = {k[len(root):] if k.startswith(root) and k[len(root):] in ("Variable", "beta1_power", "beta2_power")
               else k: v for k, v in state.items()}
        self.step.load_optimizer_state(opt)
        self.step.sync_initial_state()

    def train(self, start_epoch: int = 1, max_iters: Optional[int] = None) -> None:
        """train.py:330-338."""
        for epoch in range(start_epoch, self.max_epoch + 1):
            self.log.info("**** EPOCH %03d ****", epoch)
            self.train_one_epoch(epoch, max_iters)
