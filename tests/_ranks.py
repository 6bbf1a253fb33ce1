"""Several ranks of a row-sharded job in one process: the in-process communicator (slm_comm_init_local) makes engines of this
process the ranks of one job, each driven by its own host thread.  Shared by the row-sharded GPU tests; the row splits are
plain data, so the CPU premise tests read them too (nothing here touches the engine until ``run_ranks`` is called)."""

import threading

import numpy as np

# Explicit row counts per rank.  Ranks differ in their number of row blocks, one rank holds less than a block (1, 3, 7 rows),
# and eight ranks are the in-process communicator's most (LocalComm::kMaxRanks).
SPLITS = {
    40: [(20, 20), (39, 1), (3, 37)],
    1000: [(500, 500), (999, 1), (63, 1, 936), (333, 333, 334), (125,) * 8],
    4099: [(7, 4000, 92)],
    333: [(300, 33)],
}


def split_bounds(split):
    """[(lo, hi)] of every rank's rows."""
    edges = np.concatenate(([0], np.cumsum(split))).astype(int)
    return [(int(edges[r]), int(edges[r + 1])) for r in range(len(split))]


def run_ranks(n_ranks, work, timeout_s=30.0):
    """work(rank, engine) on n_ranks fresh engines joined by an in-process communicator; returns the results, the
    collective counts and the communicator's (rank, ranks) per engine; re-raises the first exception of any rank."""
    from sparselm_amd import _engine

    engines = [_engine.Engine(0) for _ in range(n_ranks)]
    _engine.init_local_comm(engines, timeout_s=timeout_s)
    out = [None] * n_ranks
    err = [None] * n_ranks

    def body(r):
        try:
            out[r] = work(r, engines[r])
        except BaseException as exc:  # noqa: BLE001 - reported below
            err[r] = exc

    threads = [threading.Thread(target=body, args=(r,)) for r in range(n_ranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    counts = [e.comm_collectives() for e in engines]
    infos = [e.comm_info() for e in engines]
    for e in engines:
        e.comm_destroy()
        e.close()
    for exc in err:
        if exc is not None:
            raise exc
    return out, counts, infos
