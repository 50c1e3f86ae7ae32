"""A device-resident bank of the uint8 frames the trainer has loaded (``--frame_cache_mb``).

The epoch loop touches the same files over and over: the mining cache re-embeds
``mining_cache_size`` images every ``mining_step`` anchors, the localisation check re-embeds the
references of both regions every ``eval_step`` anchors, and the per-epoch lists are the same
frames in another order.  Without the bank every one of those loads decodes the PNG, resizes it on
the host and uploads a float32 batch.  With it a frame is decoded once, kept on the device as the
uint8 pixels the loader produced (H * W * 3 bytes), and every batch is assembled there by one HIP
kernel (``scl_frames_gather``, csrc/frames.hip).  A uint8 widened to float32 on the device is the
float32 ``.astype(np.float32)`` makes on the host: the batches, and therefore the training run,
are bit-identical with and without the bank.

Three pieces:

* ``SlotMap``      key -> slot bookkeeping, pure Python.  Fixed capacity, fill-only (no eviction).
* ``FrameBank``    the device tensor; ``prepare`` (host work, any thread) + ``materialize`` (the
                   consumer's thread and stream).
* ``CachedImageSet``  an image set whose ``load_images`` goes through a bank.

A slot is free, RESERVED (a plan has promised to upload it) or COMMITTED (the upload has been
enqueued).  Only committed slots are hits: a key that an earlier, not yet materialised plan has
reserved is decoded again and travels with its own batch, so no result depends on the order in
which plans are materialised.
"""
import threading

import numpy as np


class Plan:
    """What ``SlotMap.plan`` decided for one list of keys.

    ``entries``  int32 [positions]: slot s >= 0 of the bank, or -(j + 1) for frame j of ``decode``
    ``decode``   the distinct keys to decode, in the order of their frames in the batch's ``extra``
    ``owned``    [(j, slot)]: frames of ``decode`` that were given a bank slot (reserved now)
    """

    def __init__(self, entries, decode, owned, counts):
        self.entries, self.decode, self.owned, self.counts = entries, decode, owned, counts


class SlotMap:
    """key -> slot, ``capacity`` slots, fill-only."""

    COUNTERS = ('positions', 'hits', 'decoded', 'decoded_positions', 'bypassed', 'raced')

    def __init__(self, capacity):
        self.capacity = max(int(capacity), 0)
        self._slot = {}                    # key -> slot, reserved and committed alike
        self._committed = set()            # keys whose upload has been enqueued
        self._next = 0                     # slots [0, _next) have been handed out ...
        self._free = []                    # ... except these, released by an abandoned plan
        self.stats = dict.fromkeys(self.COUNTERS, 0)

    @property
    def in_use(self):
        return len(self._slot)

    def plan(self, keys):
        """Decide where every position's frame comes from; reserves a slot for every new key the
        bank still has room for."""
        entries = np.empty(len(keys), dtype=np.int32)
        decode, owned, index = [], [], {}
        counts = dict.fromkeys(self.COUNTERS, 0)
        counts['positions'] = len(keys)
        for pos, key in enumerate(keys):
            if key in self._committed:
                entries[pos] = self._slot[key]
                counts['hits'] += 1
                continue
            j = index.get(key)
            if j is None:                  # first position of a key that must be decoded
                j = index[key] = len(decode)
                decode.append(key)
                counts['decoded'] += 1
                if key in self._slot:      # reserved by a plan that has not been materialised
                    counts['raced'] += 1
                elif self._free or self._next < self.capacity:
                    if self._free:
                        slot = self._free.pop()
                    else:
                        slot, self._next = self._next, self._next + 1
                    self._slot[key] = slot
                    owned.append((j, slot))
                else:
                    counts['bypassed'] += 1
            entries[pos] = -(j + 1)
            counts['decoded_positions'] += 1
        for name, v in counts.items():
            self.stats[name] += v
        return Plan(entries, decode, owned, counts)

    def commit(self, plan):
        """The uploads of ``plan.owned`` have been enqueued: those keys hit from now on."""
        for j, slot in plan.owned:
            key = plan.decode[j]
            if self._slot.get(key) == slot:
                self._committed.add(key)

    def release(self, plan):
        """Abandon a plan that will never be materialised: its reservations become free slots
        and its counts leave the statistics."""
        for j, slot in plan.owned:
            key = plan.decode[j]
            if self._slot.get(key) == slot and key not in self._committed:
                del self._slot[key]
                self._free.append(slot)
        for name, v in plan.counts.items():
            self.stats[name] -= v
        plan.owned = []


class PendingFrames:
    """A batch ``FrameBank.prepare`` has planned and decoded; ``materialize`` turns it into the
    float32 device tensor."""

    def __init__(self, bank, plan, new):
        self.bank, self.plan, self.new = bank, plan, new

    def __len__(self):
        return len(self.plan.entries)


def validate_entries(entries, slots, extra):
    """Every entry of a slot list points inside the bank (``slots``) or the batch's own frames
    (``extra``) — what the kernel's launcher cannot check, the list living on the device."""
    e = np.asarray(entries, dtype=np.int64)
    bad = ((e >= 0) & (e >= slots)) | ((e < 0) & (-e - 1 >= extra))
    if bad.any():
        pos = int(np.flatnonzero(bad)[0])
        raise ValueError('frame bank: slot entry %d at position %d is outside the bank (%d slots) '
                         'and the batch (%d new frames)' % (int(e[pos]), pos, slots, extra))


class FrameBank:
    """One ``uint8 [slots, H, W, 3]`` device tensor, allocated at the first frame (which fixes
    H and W; ``slots = capacity_bytes // (H * W * 3)``)."""

    def __init__(self, capacity_bytes, device):
        self.capacity_bytes = max(int(capacity_bytes), 0)
        self.device = device
        self.shape = None                  # (H, W, 3) once the first frame has been seen
        self._map = None
        self._bank = None
        self._stream = None
        self._lock = threading.Lock()
        self._uploaded = 0
        self._shape_bypass = 0

    # ---- host side -------------------------------------------------------------------------
    @property
    def slots(self):
        return 0 if self._map is None else self._map.capacity

    @property
    def stats(self):
        with self._lock:
            out = dict(self._map.stats) if self._map is not None else dict.fromkeys(SlotMap.COUNTERS, 0)
            used = self._map.in_use if self._map is not None else 0
            out.update(uploaded=self._uploaded, shape_bypassed=self._shape_bypass, slots=self.slots,
                       slots_in_use=used,
                       bytes=used * int(np.prod(self.shape)) if self.shape else 0)
        return out

    def _decode(self, image_set, indices):
        return np.ascontiguousarray(image_set.load_frames_u8(indices), dtype=np.uint8)

    def prepare(self, image_set, indices):
        """Plan the batch ``image_set[indices]`` and decode what the bank does not hold.  Host work
        only: safe on the input pipeline's worker thread.  Returns a ``PendingFrames``, or — for a
        batch whose frames do not have the bank's shape — the float32 host array
        ``image_set.load_images`` returns."""
        indices = [int(i) for i in indices]
        keys = [image_set.frame_key(i) for i in indices]
        first = {}
        for i, key in zip(indices, keys):
            first.setdefault(key, i)
        have = {}
        if self._map is None:              # the first frames fix the shape, and with it the capacity
            frames = self._decode(image_set, list(first.values()))
            have = dict(zip(first, frames))
            with self._lock:
                if self._map is None:
                    self.shape = tuple(frames.shape[1:])
                    self._map = SlotMap(self.capacity_bytes // max(int(np.prod(self.shape)), 1))
        with self._lock:
            plan = self._map.plan(keys)
        try:
            missing = [k for k in plan.decode if k not in have]
            if missing:
                have.update(zip(missing, self._decode(image_set, [first[k] for k in missing])))
            new = np.stack([have[k] for k in plan.decode]) if plan.decode else None
            if new is not None and tuple(new.shape[1:]) != self.shape:
                with self._lock:
                    self._map.release(plan)
                    self._shape_bypass += 1
                return image_set.load_images(indices)
            validate_entries(plan.entries, self.slots, len(plan.decode))
        except BaseException:
            with self._lock:
                self._map.release(plan)
            raise
        return PendingFrames(self, plan, new)

    # ---- device side -----------------------------------------------------------------------
    def materialize(self, pending):
        """float32 [n, H, W, 3] on the device, on the calling thread's current stream: the new
        frames go up once, the ones that own a slot are written into the bank and marked
        committed, then one gather kernel builds the batch."""
        import torch

        from .. import _lib
        from ..model import nets
        if pending.bank is not self:
            raise ValueError('frame bank: the batch was prepared by another bank')
        dev = self.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        if self._stream is None:
            self._stream = stream
        elif self._stream != stream:
            raise RuntimeError('frame bank: materialize() under another stream than the first '
                               'call\'s (one bank serves one stream)')
        plan, frame_bytes = pending.plan, int(np.prod(self.shape))
        if self._bank is None and self.slots > 0:
            self._bank = torch.empty((self.slots,) + self.shape, dtype=torch.uint8, device=dev)
        extra = None
        if pending.new is not None:
            extra = torch.from_numpy(pending.new).to(dev)
            # consecutive (frame, slot) pairs — all of them, unless a released slot was re-used —
            # go into the bank as one copy
            run = 0
            while run < len(plan.owned):
                end = run + 1
                while end < len(plan.owned) and plan.owned[end][0] == plan.owned[end - 1][0] + 1 \
                        and plan.owned[end][1] == plan.owned[end - 1][1] + 1:
                    end += 1
                (j, slot), c = plan.owned[run], end - run
                self._bank[slot:slot + c].copy_(extra[j:j + c])
                run = end
        with self._lock:
            self._map.commit(plan)
            self._uploaded += len(plan.decode)
        n = len(plan.entries)
        slots = torch.from_numpy(plan.entries).to(dev)
        out = torch.empty((n,) + self.shape, dtype=torch.float32, device=dev)
        _lib.check(_lib.load().scl_frames_gather(
            _lib.ptr(self._bank), self.slots if self._bank is not None else 0,
            _lib.ptr(extra), 0 if extra is None else extra.shape[0],
            _lib.ptr(slots), n, frame_bytes, _lib.ptr(out), _lib.stream_of(out)))
        nets._work('frames_gather_kernel', 0.0, 5.0 * n * frame_bytes)
        return out

    def close(self):
        """Give the device memory back (the bookkeeping goes with it)."""
        with self._lock:
            self._bank = None
            if self._map is not None:
                self._map = SlotMap(self._map.capacity)


def to_device(images, device):
    """What the training loop feeds the network: a ``PendingFrames`` is materialised by its bank,
    a float32 host array goes up as it always did."""
    import torch
    if isinstance(images, PendingFrames):
        return images.bank.materialize(images)
    return torch.from_numpy(images).to(device)


class CachedImageSet:
    """An image set (one with ``frame_key`` and ``load_frames_u8``: ``CsvImageSet``) seen through a
    ``FrameBank``: the interface the epoch loop touches, with ``load_images`` returning what
    ``to_device`` takes."""

    def __init__(self, image_set, bank):
        self.image_set, self.bank = image_set, bank

    @property
    def xy(self):
        return self.image_set.xy

    @property
    def yaw(self):
        return self.image_set.yaw

    def __len__(self):
        return len(self.image_set)

    def __getattr__(self, name):           # path, meta, ...: whatever else the set offers
        return getattr(self.image_set, name)

    def load_raw(self, i):
        return self.image_set.load_raw(i)

    def load_images(self, indices):
        return self.bank.prepare(self.image_set, indices)


def wrap(image_set, bank):
    """``image_set`` behind ``bank`` when there is a bank and the set has frame keys (the synthetic
    set's pixels are not integers: it has none and stays as it is)."""
    if bank is None or not hasattr(image_set, 'frame_key'):
        return image_set
    return CachedImageSet(image_set, bank)
