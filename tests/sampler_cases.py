"""What the sampler tests share: a KG's sampling context on the host and on the device, and the full expected output of a
two-KG launch from the C restatement of the specification (oracle/mke_oracle.c, itself held to oracle/sampler_oracle.py by
tests/test_sampler_oracle.py)."""
import numpy as np
import torch

from oracle import c_oracle as co
from oracle import sampler_oracle as so


def dev(a, dtype=np.int32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")


class Side:
    """One KG's sampling context, on the host (for the specification and its C restatement) and on the device."""

    def __init__(self, ents, known=None, cand_table=None, cand_valid=None):
        from multike_amd.sampling import KGSide, KnownTripleSet
        self.ents = np.ascontiguousarray(ents, dtype=np.int64)
        self.contiguous = bool(np.array_equal(self.ents, np.arange(self.ents[0], self.ents[0] + len(self.ents))))
        self.cand_table, self.cand_valid = cand_table, cand_valid
        self.set_host_known(known)
        self.ks = None if known is None else KnownTripleSet(*(dev(self.known_np[:, k]) for k in range(3)))
        self.dev = KGSide(self.ents, self.ks)
        if cand_table is not None:
            self.dev.set_neighbours(dev(cand_table), None if cand_valid is None else dev(cand_valid, np.uint8))

    def set_host_known(self, known):
        """The known triples the host side answers by (the device set is the caller's to keep in step)."""
        self.known_np = None if known is None else np.asarray(known, dtype=np.int32)
        self.known_py = None if known is None else {tuple(x) for x in self.known_np.tolist()}
        self.known_c = None if known is None else co.TripleSet(*(self.known_np[:, k] for k in range(3)))

    def _population(self):
        return dict(ent_lo=int(self.ents[0]) if self.contiguous else 0, ent_list=None if self.contiguous else self.ents,
                    cand_table=self.cand_table, cand_valid=self.cand_valid)

    def spec(self, h, r, t, N, seed, stream_id, gi, max_try):
        """The Python specification's negatives of ONE positive at stream position gi."""
        return so.philox_negatives([h], [r], [t], N, len(self.ents), known=self.known_py, seed=seed, stream_id=stream_id, pos_offset=gi,
                                   max_try=max_try, **self._population())

    def restated(self, pos, N, seed, stream_id, pos_index, max_try):
        """The C restatement's negatives of the positives `pos` at the stream positions pos_index."""
        return co.neg_sample(*pos, N, len(self.ents), known=self.known_c, seed=seed, stream_id=stream_id, pos_index=pos_index,
                             max_try=max_try, **self._population())


def expected_negatives(pos, kg, sides, N, pos_index, max_try, seed, sid):
    """(neg_h, neg_r, neg_t), each [n_pos, N], of a launch over `sides` (one, or one per KG; positive i is of KG kg[i] != 0, of
    the first when kg is None) with positive i at stream position pos_index[i]: one call of the C restatement per KG, on that
    KG's positives with their own positions and the KG's stream (sid + KG), scattered back."""
    n = len(pos[0])
    which = np.zeros(n, bool) if kg is None else np.asarray(kg) != 0
    out = [np.full((n, N), -1, np.int32) for _ in range(3)]
    for k in (0, 1):
        rows = np.flatnonzero(which == bool(k))
        if len(rows) == 0:
            continue
        got = sides[k if len(sides) > 1 else 0].restated([np.asarray(x)[rows] for x in pos], N, seed, sid + k, np.asarray(pos_index)[rows], max_try)
        for a, g in zip(out, got):
            a[rows] = g.reshape(len(rows), N)
    return out
