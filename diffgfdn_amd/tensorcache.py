"""Device-side constants memoised by the IDENTITY of the tensors they were built from: the one rule, for every such cache.

A tensor is identified by ``tensor_key``: address, shape, stride, dtype, device and version counter -- no host sync, no read of
the device.  An address identifies a tensor only while that tensor is alive, so an entry holds its key tensors strongly: the
allocator cannot hand their blocks to other tensors while the entry exists (a freed grid's address reused by another grid was
a false hit once: wrong phasors, H off by 4e-3 in one test order), and an in-place edit moves the version counter.
Eviction drops the OLDEST entry, one at a time, and never clears: a cache cleared during the warm-up of a later step rebuilt
the earlier steps' entries, with their host reads, inside the capture (hipErrorStreamCaptureUnsupported)."""
import torch


def tensor_key(t):
    return None if t is None else (t.data_ptr(), tuple(t.shape), t.stride(), t.dtype, t.device, t._version)


def _capturing() -> bool:
    return torch.cuda.is_initialized() and torch.cuda.is_current_stream_capturing()


class TensorCache:
    """``get(tensors, extra, build)`` -> the value built for these tensors (each a tensor or None) and the hashable ``extra``.

    capacity:   entries kept; at ``capacity=1`` the old entry is released BEFORE ``build()`` runs (never two stores alive).
    by_value:   on an identity miss, an entry with the same ``extra`` whose tensors had equal shape, dtype, device and values
                (against copies taken when it was built) is a hit, and is re-keyed to the new tensors.  A hit by identity
                compares nothing.
    no_capture: message of the RuntimeError raised when a build is attempted inside a stream capture."""

    def __init__(self, capacity: int = 1, by_value: bool = False, no_capture: str = None):
        self.capacity, self.by_value, self.no_capture = capacity, by_value, no_capture
        self._entries = {}                       # key -> (value, key tensors, their copies or None), oldest first

    def get(self, tensors, extra, build):
        tensors = tuple(tensors)
        key = (tuple(tensor_key(t) for t in tensors), extra)
        entry = self._entries.get(key)
        if entry is None and self.by_value:
            entry = self._rekey_equal(key, tensors)
        if entry is None:
            if self.no_capture is not None and _capturing():
                raise RuntimeError(self.no_capture)
            while len(self._entries) >= self.capacity:
                del self._entries[next(iter(self._entries))]
            copies = tuple(None if t is None else t.detach().clone() for t in tensors) if self.by_value else None
            entry = self._entries[key] = (build(), tensors, copies)
        return entry[0]

    def _rekey_equal(self, key, tensors):
        for old, (value, _, copies) in self._entries.items():
            if old[1] == key[1] and len(copies) == len(tensors) and all(
                    (c is None and t is None) or (c is not None and t is not None and c.shape == t.shape
                                                  and c.dtype == t.dtype and c.device == t.device and torch.equal(c, t))
                    for c, t in zip(copies, tensors)):
                del self._entries[old]
                entry = self._entries[key] = (value, tensors, copies)
                return entry
        return None

    def values(self):
        return [e[0] for e in self._entries.values()]

    def clear(self):
        self._entries.clear()
