"""Device buffers between guard bands, for the tests that hand a C entry point EXACTLY the bytes its
size query returned: the bytes on either side must come back untouched, and a run on a buffer full of
FILL must equal a run on a zeroed one — nothing is read before it is written."""
import torch

GUARD, FILL = 4096, 0xA5


class Guarded:
    """``nbytes`` device bytes (``.inner``) between two guard bands, all filled with ``fill``."""

    def __init__(self, dev, nbytes, fill):
        self.fill = fill
        self.buf = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device=dev)
        self.inner = self.buf[GUARD:GUARD + nbytes]
        assert self.inner.data_ptr() % 256 == 0 and self.inner.numel() == nbytes

    def assert_bands_intact(self):
        torch.cuda.synchronize()
        assert bool((self.buf[:GUARD] == self.fill).all()), "bytes before the block were written"
        assert bool((self.buf[-GUARD:] == self.fill).all()), "bytes behind the block were written"
