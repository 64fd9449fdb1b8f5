"""Notes as columns: what the note ops (piano rolls, rendering, note matching, the target tokenizer) share on the host --
one extraction of a NoteSequence's fields, one check of times and of MIDI ranges, offset tables, and the one upload of a
job's packed columns.  Numpy only, but for `to_device` / `upload`."""
import operator

import numpy as np

# what each field of a Note is read as; is_drum is read as bool(x) and, like every whole number, returned as int64
_READ = {"start_time": np.float64, "end_time": np.float64, "pitch": np.int64, "velocity": np.int64, "is_drum": np.bool_,
         "program": np.int64}


def fields(seq, program=False) -> tuple:
    """(start f64, end f64, pitch i64, velocity i64, is_drum i64[, program i64]) of one NoteSequence (is_drum 0 / 1), or of
    a record array with those field names (metrics_utils.NOTE_DTYPE: what metrics_utils.decode_token_rows returns)"""
    out = []
    for name, read in list(_READ.items())[:6 if program else 5]:
        column = seq[name] if isinstance(seq, np.ndarray) else \
            np.fromiter(map(operator.attrgetter(name), seq.notes), read, len(seq.notes))
        out.append(column.astype(np.float64 if read is np.float64 else np.int64))
    return tuple(out)


def check_times(*times, not_negative=False, prefix="") -> None:
    """ValueError(prefix + "note times must be finite[ and not negative]") unless every value of every array is"""
    if not all(np.isfinite(t).all() and not (not_negative and (t < 0).any()) for t in times):
        raise ValueError(prefix + "note times must be finite" + (" and not negative" if not_negative else ""))


def check_range(message, *columns, got=True) -> None:
    """ValueError(message[ + ", got <the first offender>"]) unless every value of every column is a MIDI value, 0 .. 127"""
    for c in columns:
        bad = (c < 0) | (c > 127)
        if bad.any():
            raise ValueError(message + (", got %d" % c[bad][0] if got else ""))


def offsets(lengths) -> np.ndarray:
    """int64 [n + 1]: 0, then the running sums of `lengths`; offsets(...)[:-1] is where each item starts"""
    return np.concatenate([np.zeros(1, np.int64), np.cumsum(np.asarray(lengths, np.int64))])


def column_offsets(itemsizes, n) -> list:
    """the byte offset of every column of `n` items when the columns lie back to back.  ValueError if one would start at
    an address that is no multiple of its item size"""
    out = [n * sum(itemsizes[:k]) for k in range(len(itemsizes))]
    for k, (at, size) in enumerate(zip(out, itemsizes)):
        if at % size:
            raise ValueError("column %d (%d-byte items) would start at byte %d: put wider columns first" % (k, size, at))
    return out


def pack(columns, dtypes) -> np.ndarray:
    """one uint8 buffer of the columns back to back, the form `upload` takes; column k is the concatenation of the arrays
    columns[k] as dtypes[k] (explicit little-endian)"""
    cols = [np.concatenate(c).astype(dt) if c else np.zeros(0, dt) for c, dt in zip(columns, dtypes)]
    column_offsets([c.itemsize for c in cols], len(cols[0]))
    return np.concatenate([c.view(np.uint8) for c in cols])


def to_device(array):
    """`array` as a CUDA tensor, uploaded on the current stream and recorded on it: the one policy of the note ops"""
    import torch
    t = torch.from_numpy(array).cuda()
    t.record_stream(torch.cuda.current_stream())
    return t


def one_buffer(tensors):
    """the files' float32 [rows, mel] blocks as ONE device buffer: as they lie when each starts where the one before it
    ends (slices of one tensor: the engine's job) -- then the FIRST block, whose storage the others continue -- else one
    torch.cat"""
    import torch
    if all(b.data_ptr() == a.data_ptr() + a.numel() * 4 for a, b in zip(tensors, tensors[1:])):
        return tensors[0]
    return torch.cat([t.reshape(-1, t.shape[-1]) for t in tensors], 0)


def upload(packed, n, dtypes) -> tuple:
    """ONE upload of a job's columns, `n` items each, `packed` back to back as `dtypes` -> (the tensor that owns them, the
    device address of every column); no items: (None, [None] * k) and nothing is uploaded"""
    if n == 0:
        return None, [None] * len(dtypes)
    notes = to_device(packed)
    return notes, [notes.data_ptr() + at for at in column_offsets([np.dtype(dt).itemsize for dt in dtypes], n)]
