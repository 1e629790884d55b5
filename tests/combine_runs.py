"""Run directories for the `kmx combine` tests, written by hand from combine_ref blocks: options.txt, hash.info, the repartition
table, kmtricks.fof and one matrix per partition (or, for a run that still holds its count files, one .kmer file per sample)."""
import os, re, struct
import numpy as np

import combine_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KMX = os.path.join(ROOT, "kmtricks_amd", "kmx")
KM_BASE = struct.pack("<QIB", 0x736b636972746d6b, 0, 0)
KINDS = ("count", "pa", "count_hash", "pa_hash")


def magics():
    src = open(os.path.join(ROOT, "kmtricks_amd", "host", "kmx_io.hpp")).read()
    return {n.lower(): int(v, 16) for n, v in re.findall(r"MAGIC_(\w+) = (0x[0-9a-fA-F]+)ULL", src)}


def matrix_header(kind, k, n_cols, sid, part):
    M, slots = magics(), (k + 31) // 32
    if kind == "count":
        return KM_BASE + struct.pack("<QIIIIII", M["matrix"], k, slots, 1, n_cols, sid, part)
    if kind == "count_hash":
        return KM_BASE + struct.pack("<QIIII", M["matrix_hash"], 4, n_cols, sid, part)
    if kind == "pa":
        return KM_BASE + struct.pack("<QIIIIII", M["pa"], k, slots, n_cols, (n_cols + 7) // 8, sid, part)
    return KM_BASE + struct.pack("<QIIII", M["pa_hash"], n_cols, (n_cols + 7) // 8, sid, part)


def header_bytes(kind):
    return 45 if kind in ("count", "pa") else 37


def kmer_header(k, count_bytes, sid, part):
    return KM_BASE + struct.pack("<QIIIII", magics()["kmer"], k, (k + 31) // 32, count_bytes, sid, part)


def write_layout(root, kind, P, ids):
    for s in ("matrices", "repartition_gatb", "config_gatb", "counts/partition_0"):
        os.makedirs(f"{root}/{s}")
    open(f"{root}/repartition_gatb/repartition.minimRepart", "wb").write(b"same table" * 10)
    open(f"{root}/config_gatb/gatb.config", "wb").write(b"cfg")
    open(f"{root}/hash.info", "wb").write(struct.pack("<QQQQQ", 1000, P, 10, 2, 10))
    mode = "pa" if kind.startswith("pa") else "count"
    fmt = "hash" if kind.endswith("hash") else "kmer"
    open(f"{root}/options.txt", "w").write(f"Options: dir={root}, verbosity=info, nb_threads=1, mode={mode}, format=bin, bf_format=howdesbt, count_format={fmt}, until=all\n")
    open(f"{root}/kmtricks.fof", "w").write("".join(f"{i}: /x/{i}.fa\n" for i in ids))


def write_run(root, kind, k, blocks, ids, sid=7):
    """a run with one matrix per partition: blocks[p] = (keys, payload, n_cols, 4) of combine_ref"""
    write_layout(root, kind, len(blocks), ids)
    for p, b in enumerate(blocks):
        open(f"{root}/matrices/matrix_{p}.{kind}", "wb").write(matrix_header(kind, k, b[2], sid, p) + cr.block_body(b[0], b[1]))


def write_count_run(root, k, samples, ids):
    """a run that still holds its count files: samples[s][p] = (keys, payload, 1, count_bytes), one .kmer file per sample and partition"""
    P = len(samples[0])
    write_layout(root, "count", P, ids)
    for p in range(P):
        os.makedirs(f"{root}/counts/partition_{p}", exist_ok=True)
        for s, parts in enumerate(samples):
            b = parts[p]
            open(f"{root}/counts/partition_{p}/{ids[s]}.kmer", "wb").write(kmer_header(k, b[3], s, p) + cr.block_body(b[0], b[1]))


def tree(root):
    """every file under root -> its bytes"""
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            path = os.path.join(d, f)
            out[os.path.relpath(path, root)] = open(path, "rb").read()
    return out
