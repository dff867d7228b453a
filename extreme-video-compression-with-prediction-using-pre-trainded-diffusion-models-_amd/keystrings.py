"""The strings of key frames: ``[y_strings[5][2][B], z_strings[B]]``, y strings by slice, pass and clip, z strings by clip
(``ElicModel.compress`` writes the structure, ``decompress`` reads it; B = 1 is the per-frame entry of a job stream).

Everything that walks the structure is here, once: splitting a batch into frames and merging frames into a batch, the bit
count, the identity of a frame's strings, and the one order in which the container formats serialise them."""
import struct

N_SLICES, N_PASSES = 5, 2


def split(strings):
    """A batch -> per clip, the strings of that clip alone (B = 1)."""
    ys, zs = strings
    return [[[[[p[b]] for p in sl] for sl in ys], [zs[b]]] for b in range(len(zs))]


def merge(parts):
    """Frames (or batches) -> one batch, their clips concatenated in the given order."""
    ys = [[[s for k in parts for s in k[0][sl][p]] for p in range(N_PASSES)] for sl in range(len(parts[0][0]))]
    return [ys, [s for k in parts for s in k[1]]]


def bits(strings):
    """8 x the bytes of every string, of one structure or of any nesting of them (the reference counts the same,
    Inference.py:51-67)."""
    return sum(bits(s) for s in strings) if isinstance(strings, (list, tuple)) else 8 * len(strings)


def flat(strings):
    """The strings as one tuple of bytes: what makes two key frames of one q the same frame."""
    return tuple(s for sl in strings[0] for p in sl for s in p) + tuple(strings[1])


class Reader:
    """A cursor over a stream's bytes that refuses to run past their end.  ``noun`` ("container", "job stream") words the
    errors."""

    def __init__(self, blob, off, noun):
        self.blob, self.off, self.noun = blob, off, noun

    def need(self, n):
        if self.off + n > len(self.blob):
            raise ValueError(f"truncated {self.noun}")

    def unpack(self, fmt):
        self.need(struct.calcsize(fmt))
        values = struct.unpack_from(fmt, self.blob, self.off)
        self.off += struct.calcsize(fmt)
        return values

    def take(self):
        """``u32 len | bytes`` -> the bytes."""
        (n,) = self.unpack("<I")
        self.need(n)
        self.off += n
        return bytes(self.blob[self.off - n:self.off])

    def end(self):
        if self.off != len(self.blob):
            raise ValueError(f"trailing bytes in {self.noun}")


def write(out, strings, b=0):
    """Append clip b of ``strings`` to the list of byte pieces ``out``: z, then slice 0..4 x pass 0..1, each ``u32 len | bytes``."""
    ys, zs = strings
    for s in [zs[b]] + [ys[i][p][b] for i in range(N_SLICES) for p in range(N_PASSES)]:
        out.append(struct.pack("<I", len(s)) + s)


def read(reader, n_clips=1):
    """What ``write`` wrote for clips 0 .. n_clips - 1, one after the other -> the batch."""
    clips = [[reader.take() for _ in range(1 + N_SLICES * N_PASSES)] for _ in range(n_clips)]
    ys = [[[c[1 + i * N_PASSES + p] for c in clips] for p in range(N_PASSES)] for i in range(N_SLICES)]
    return [ys, [c[0] for c in clips]]
