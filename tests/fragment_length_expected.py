"""The whole-file probes of the reference (rocco/native/ccounts_backend.c: ccounts_isPairedEnd 598-652,
ccounts_getReadLength 654-856, ccounts_getFragmentLength 861-1524, ccounts_getMappedReadCount 1712-1888) and the body of
``_get_bam_count_metadata`` (rocco/readtracks.py:242-353), stated in NumPy over decoded records -- the statement the
fixtures pin (tests/test_fragment_length_host.py) and the device code is compared with (tests/test_gpu_fragment_length.py).

A file is ``(contigs, records)``: ``contigs`` the header's ``(name, length)`` pairs in header order, ``records[name]`` a dict
of the seven arrays ``pos end isize flag mapq mate_same qlen`` in file order.  A lag score is ``np.cumsum(a * b)[-1]``:
``cumsum`` adds in order, one product after the other, as the reference's loop does (``np.sum`` and ``np.dot`` do not)."""
import numpy as np

FIELDS = ("pos", "end", "isize", "flag", "mapq", "mate_same", "qlen")


def file_order(file, names=None):
    """The seven arrays of the file's records in file order (header order), or of the contigs ``names`` in their order."""
    contigs, records = file
    order = [n for n, _ in contigs] if names is None else names
    parts = [records[n] for n in order if n in records and len(records[n]["pos"])]
    return {f: (np.concatenate([p[f] for p in parts]) if parts else np.zeros(0, dtype=np.int64)).astype(np.int64) for f in FIELDS}


def uint_median(values):
    v = np.sort(np.asarray(values, dtype=np.int64))
    mid = v.size // 2
    return int((v[mid - 1] + v[mid]) // 2) if v.size % 2 == 0 else int(v[mid])


def is_paired_end(file, max_reads=1000):
    flags = file_order(file)["flag"]
    if max_reads > 0:
        flags = flags[:max_reads]
    return bool(np.any(flags & 1))


def read_length(file, min_reads=32, max_iterations=4096, flag_exclude=0):
    min_reads = max(min_reads, 1)
    max_iterations = max(max_iterations, min_reads)
    r = file_order(file)
    flags, qlen = r["flag"][:max_iterations], r["qlen"][:max_iterations]
    good = qlen[((flags & flag_exclude) == 0) & (qlen > 0)][:min_reads]
    if good.size == 0:
        raise RuntimeError("failed to estimate read length")
    return uint_median(good)


def mapped_read_count(file, exclude=()):
    contigs, records = file
    mapped = unmapped = 0
    for name, _ in contigs:
        if name in exclude or name not in records:
            continue
        flags = np.asarray(records[name]["flag"]).astype(np.int64)
        mapped += int(np.count_nonzero((flags & 4) == 0))
        unmapped += int(np.count_nonzero(flags & 4))
    return mapped, unmapped


def top_contigs(contigs):
    """ccounts_backend.c:994-1013."""
    top_len, top_name = [0, 0, 0], [None, None, None]
    for name, length in contigs:
        for i in range(3):
            if length > top_len[i]:
                for j in range(2, i, -1):
                    top_len[j], top_name[j] = top_len[j - 1], top_name[j - 1]
                top_len[i], top_name[i] = length, name
                break
    return [(n, length) for n, length in zip(top_name, top_len) if n is not None and length > 0]


def clamp_parameters(flag_exclude=0, max_iterations=1000, max_insert_size=1000, block_size=5000, rolling_chunk_size=250, lag_step=5,
                     early_exit=250, fallback=0):
    """ccounts_backend.c:940-967."""
    p = dict(flag_exclude=flag_exclude, max_iterations=max(max_iterations, 1), max_insert_size=max(max_insert_size, 1),
             block_size=max(block_size, 64), rolling_chunk_size=max(rolling_chunk_size, 1), lag_step=max(lag_step, 1),
             early_exit=early_exit, fallback=fallback if fallback > 0 else 0)
    if p["early_exit"] < 1:
        p["early_exit"] = p["max_iterations"]
    return p


def sample_pass(file, top, flag_exclude, max_iterations):
    """ccounts_backend.c:1015-1060: (records sampled, sum of their query lengths, pairedEnd)."""
    r = file_order(file, [n for n, _ in top])
    count, total, paired = 0, 0.0, False
    for flag, qlen in zip(r["flag"].tolist(), r["qlen"].tolist()):
        if count >= max_iterations:
            break
        if flag & flag_exclude or flag & 4:
            continue
        if flag & 1:
            paired = True
        if qlen <= 0:
            continue
        total += float(qlen)
        count += 1
    return count, total, paired


def window_size(block_size, rolling_chunk_size):
    win = max(block_size // rolling_chunk_size, 1)
    return win + 1 if win % 2 == 0 else win


def chunk_density(pos, flag, contig_length, flag_exclude, block_size, rolling_chunk_size):
    """ccounts_backend.c:1217-1311: the window sums (as integers; the reference holds them in doubles, exact below 2**53)."""
    num_chunks = (contig_length + rolling_chunk_size - 1) // rolling_chunk_size
    pos, flag = np.asarray(pos).astype(np.int64), np.asarray(flag).astype(np.int64)
    keep = ((flag & flag_exclude) == 0) & ((flag & 4) == 0) & (pos < contig_length)
    cells = pos[keep] // rolling_chunk_size
    raw = np.bincount(cells[cells < num_chunks], minlength=num_chunks).astype(np.int64)
    prefix = np.concatenate([[0], np.cumsum(raw)])
    win = window_size(block_size, rolling_chunk_size)
    start = np.arange(num_chunks) - win // 2
    end = start + win
    low = start < 0
    start, end = np.where(low, 0, start), np.where(low, min(win, num_chunks), end)
    high = end > num_chunks
    end = np.where(high, num_chunks, end)
    start = np.where(high, np.maximum(end - win, 0), start)
    return prefix[end] - prefix[start]


def ranking(density):
    """ccounts_backend.c:1313: value descending, index ascending."""
    return np.lexsort((np.arange(density.size), -density))


def pick_centers(density, order, block_size, rolling_chunk_size, max_iterations):
    """ccounts_backend.c:1314-1339."""
    n = density.size
    win = window_size(block_size, rolling_chunk_size)
    take = min(max_iterations, n)
    seen = np.zeros(n, dtype=bool)
    centers = []
    for index in order.tolist():
        if len(centers) >= take:
            break
        if density[index] <= 0:  # (descending: nothing positive follows)
            break
        if seen[index]:
            continue
        centers.append(index)
        start = max(index - win // 2, 0)
        seen[start: min(index - win // 2 + win, n)] = True
    return np.asarray(centers, dtype=np.int64)


def block_start(center, contig_length, block_size, rolling_chunk_size):
    """ccounts_backend.c:1343-1359; None where the reference skips the block."""
    start = max(center * rolling_chunk_size + rolling_chunk_size // 2 - block_size // 2, 0)
    if start + block_size > contig_length:
        start = contig_length - block_size
        if start < 0:
            return None
    return start


def xcorr_block(records, start, block_size, flag_exclude, min_lag, max_insert_size, lag_step):
    """ccounts_backend.c:1361-1469 for the block [start, start + block_size): (best_lag, best_score, fwd_sum, rev_sum);
    best_lag -1 and best_score 0.0 where the reference leaves the block before its lag loop."""
    pos, end, flag = (np.asarray(records[f]).astype(np.int64) for f in ("pos", "end", "flag"))
    stop = start + block_size
    # what the index iterator over [start, stop) yields, and the two containment tests
    keep = (pos < stop) & (end > start) & ((flag & flag_exclude) == 0) & ((flag & 4) == 0) & (end > pos) & (pos >= start) & (end <= stop)
    reverse = (flag & 16) != 0
    fwd = np.bincount(pos[keep & ~reverse] - start, minlength=block_size).astype(np.float64)
    rev = np.bincount(end[keep & reverse] - 1 - start, minlength=block_size).astype(np.float64)
    fwd_sum, rev_sum = int(fwd.sum()), int(rev.sum())
    last_lag = min(max_insert_size, block_size - 1)
    if fwd_sum < 10 or rev_sum < 10 or last_lag < min_lag:
        return -1, 0.0, fwd_sum, rev_sum
    fwd = fwd - float(fwd_sum) / float(block_size)
    rev = rev - float(rev_sum) / float(block_size)
    scores = lag_scores(fwd, rev, np.arange(min_lag, last_lag + 1, lag_step))
    best_lag, best_score = -1, 0.0
    for lag, score in zip(range(min_lag, last_lag + 1, lag_step), scores.tolist()):
        if best_lag < 0 or score > best_score:
            best_lag, best_score = lag, score
    return best_lag, best_score, fwd_sum, rev_sum


def lag_scores(fwd, rev, lags):
    """score[l] = np.cumsum(fwd[:n - lag] * rev[lag:])[-1] for every lag at once: row l holds the products of lag l, padded
    with +0.0 behind its n - lag entries (adding +0.0 leaves every partial sum as it is, and a partial sum is never -0.0),
    and cumsum runs along each row in order."""
    n = fwd.size
    index = np.arange(n)[None, :] + np.asarray(lags)[:, None]
    products = np.where(index < n, fwd[None, :] * rev[np.minimum(index, n - 1)], 0.0)
    return np.cumsum(products, axis=1)[:, -1]


def fragment_length(file, details=None, cache=None, **parameters):
    """ccounts_getFragmentLength.  ``details`` (a dict) receives what the run went through; ``cache`` (a dict the caller keeps
    for ONE file) remembers the blocks already correlated, so that scenarios over the same blocks share them."""
    p = clamp_parameters(**parameters)
    contigs, records = file
    top = top_contigs(contigs)
    count, total, paired = sample_pass(file, top, p["flag_exclude"], p["max_iterations"])
    result = p["fallback"]
    if details is not None:
        details.update(sampled=count, paired=paired, candidates=[], blocks=[])
    if count <= 0:
        return result
    min_insert = min(max(int(total / float(count)), 1), p["max_insert_size"])
    if details is not None:
        details["min_insert"] = min_insert
    if paired:
        required = max(p["max_iterations"], 2000)
        r = file_order(file, [n for n, _ in top])
        flag, length = r["flag"], np.abs(r["isize"])
        keep = (((flag & p["flag_exclude"]) == 0) & ((flag & 2) != 0) & ((flag & 128) == 0) & ((flag & 8) == 0) & (r["mate_same"] != 0)
                & (length >= min_insert) & (length <= p["max_insert_size"]))
        lengths = length[keep][:required]
        if details is not None:
            details["templates"] = int(lengths.size)
        if lengths.size:
            result = min(max(uint_median(lengths), min_insert), p["max_insert_size"])
        return result
    lags = []
    for name, contig_length in top:
        if len(lags) >= p["early_exit"]:
            break
        if contig_length < p["block_size"]:
            continue
        empty = {f: np.zeros(0, dtype=np.int64) for f in FIELDS}
        rec = records.get(name, empty)
        density = chunk_density(rec["pos"], rec["flag"], contig_length, p["flag_exclude"], p["block_size"], p["rolling_chunk_size"])
        centers = pick_centers(density, ranking(density), p["block_size"], p["rolling_chunk_size"], p["max_iterations"])
        before = len(lags)
        for center in centers.tolist():
            if len(lags) >= p["early_exit"]:
                break
            start = block_start(center, contig_length, p["block_size"], p["rolling_chunk_size"])
            if start is None:
                continue
            key = (name, start, p["block_size"], p["flag_exclude"], min_insert, p["max_insert_size"], p["lag_step"])
            if cache is None or key not in cache:
                block = xcorr_block(rec, start, p["block_size"], p["flag_exclude"], min_insert, p["max_insert_size"], p["lag_step"])
                if cache is not None:
                    cache[key] = block
            best_lag, best_score, _, _ = block if cache is None else cache[key]
            if best_lag > 0 and best_score != 0.0:
                lags.append(best_lag + 1)
        if details is not None:
            details["candidates"].append(len(lags) - before)
            details["blocks"].append(int(centers.size))
    if lags:
        result = min(max(uint_median(lags), min_insert), p["max_insert_size"])
    return result


def native_scale_factor(norm_method, effective_genome_size, step, mapped_reads, norm_read_length, scale_factor=1.0):
    """rocco/readtracks.py:210-239."""
    method = "" if norm_method is None else norm_method.lower().replace(" ", "").upper()
    mapped = max(int(mapped_reads), 1)
    scale = float(scale_factor)
    if method == "RPGC":
        if effective_genome_size is None or float(effective_genome_size) <= 0:
            raise ValueError("Effective genome size must be positive for RPGC normalization.")
        coverage = (float(mapped) * float(max(int(norm_read_length), 1))) / float(effective_genome_size)
        return float(scale * (1.0 / max(coverage, 1.0e-12)))
    if method == "RPKM":
        return float(scale * (1.0 / max((float(mapped) / 1.0e6) * (float(step) / 1000.0), 1.0e-12)))
    if method in {"CPM", "BPM"}:
        return float(scale * (1.0 / max(float(mapped) / 1.0e6, 1.0e-12)))
    raise ValueError(f"Normalization method must be one of `RPGC`, `RPKM`, `CPM`, or `BPM`, not `{norm_method}`.")


def count_metadata(file, step, norm_method, effective_genome_size, ignore_for_norm, flag_exclude=0, extend_reads=-1, scale_factor=1.0,
                   bam_file="{file}", cache=None):
    """rocco/readtracks.py:269-351: (the dict without ``threads``, the log records as [level, message])."""
    log = []
    paired_end = is_paired_end(file, max_reads=1024)
    length = read_length(file, min_reads=32, max_iterations=4096, flag_exclude=max(0, flag_exclude))
    mapped, _ = mapped_read_count(file, tuple(ignore_for_norm or []))
    norm_read_length, resolved, paired_end_mode = length, int(extend_reads), False
    if extend_reads == 0:
        fragment = fragment_length(file, cache=cache, flag_exclude=max(0, flag_exclude), max_iterations=4096, fallback=0)
        fragment = fragment if fragment > 0 else None
        if paired_end:
            if fragment is not None:
                norm_read_length, paired_end_mode, resolved = fragment, True, 0
            else:
                log.append(["WARNING", f"Could not estimate fragment length for {bam_file}; falling back to read length {length}."])
        elif fragment is not None and fragment > length:
            norm_read_length = resolved = fragment
            log.append(["INFO", f"Using inferred single-end fragment length {fragment} for {bam_file}."])
        else:
            log.append(["WARNING", f"`extend_reads=0` requests fragment-length inference, but {bam_file} did not yield a larger "
                                   f"single-end fragment length; using read length {length}."])
            resolved = -1
    elif extend_reads > 0:
        norm_read_length = resolved = int(extend_reads)
    scale = native_scale_factor(norm_method, effective_genome_size, step, mapped, norm_read_length, scale_factor)
    return ({"paired_end": paired_end, "paired_end_mode": paired_end_mode, "read_length": int(length),
             "norm_read_length": int(norm_read_length), "resolved_extend_bp": int(resolved), "mapped_reads": int(mapped),
             "norm_scale": float(scale)}, log)
