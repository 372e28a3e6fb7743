"""Mirror of tapir/db.py: the phylogenetic-informativeness.sqlite writer.

The DDL strings are the reference's own (tapir/db.py:19-30), whitespace included, because sqlite stores
them verbatim in sqlite_master.sql and the drop-in contract is a byte-identical schema.  Differences:
rows go in with executemany inside one transaction (the reference issues one execute per row, :51-60), and
an existing database is replaced without the interactive prompt (the reference's prompt always answers
yes: `answer == "Y" or "YES"`, :34)."""
import os
import sqlite3

DDL = [
    "CREATE TABLE loci (id INTEGER PRIMARY KEY AUTOINCREMENT, locus TEXT)",
    '''CREATE TABLE net (id INT, time INT, pi FLOAT,
            FOREIGN KEY(id) REFERENCES loci(id) DEFERRABLE INITIALLY
            DEFERRED)''',
    '''CREATE TABLE discrete (id INT, time INT, pi FLOAT, 
            FOREIGN KEY(id) REFERENCES loci(id) DEFERRABLE INITIALLY
            DEFERRED)''',
    '''CREATE TABLE interval (id INT, interval TEXT, pi FLOAT,
            error FLOAT, FOREIGN KEY(id) REFERENCES loci(id) DEFERRABLE
            INITIALLY DEFERRED)''',
]


def create_probe_db(db_name):
    """Create the four tables; returns (conn, cursor) like tapir/db.py:15-42."""
    if os.path.exists(db_name):
        os.remove(db_name)
    conn = sqlite3.connect(db_name)
    c = conn.cursor()
    c.execute("PRAGMA foreign_keys = ON")
    for stmt in DDL:
        c.execute(stmt)
    return conn, c


def locus_name(path):
    """Name stored in loci.locus: basename minus its last extension (tapir/db.py:47-48)."""
    return os.path.splitext(os.path.basename(path))[0]


def insert_pi_data(conn, c, pis):
    """pis: iterable of worker()-style tuples (name, rates, mean_rate, pi, pi_net, times, epochs); only
    name, pi_net, times and epochs are stored (tapir/db.py:44-61)."""
    for locus in pis:
        name, rates, mean_rate, pi, pi_net, times, epochs = locus
        c.execute("INSERT INTO loci(locus) VALUES (?)", (locus_name(name),))
        key = c.lastrowid
        c.executemany("INSERT INTO net VALUES (?,?,?)", [(key, k, float(v)) for k, v in enumerate(pi_net)])
        if times:
            c.executemany("INSERT INTO discrete VALUES (?,?,?)", [(key, int(k), float(v)) for k, v in times.items()])
        if epochs:
            c.executemany("INSERT INTO interval VALUES (?,?,?,?)",
                          [(key, k, float(v['sum(integral)']), float(v['sum(error)'])) for k, v in epochs.items()])
    return


def insert_tables(conn, c, names, tables, T, times, intervals):
    """Bulk form for the batch engine: tables[l] = [net(T) | disc(n_t) | integral(n_i) | error(n_i)].  One executemany per
    table over columns prepared with numpy (C4: 5.4 M rows; a list comprehension per locus was half of the stage's time).
    Row order inside each table is locus by locus, as the reference's loop writes them (tapir/db.py:44-61)."""
    import numpy as np
    L = len(names)
    if L == 0:
        return
    n_t, n_i = len(times), len(intervals)
    labels = ["{0}-{1}".format(a, b) for a, b in intervals]
    tables = np.asarray(tables, dtype=np.float64)
    c.executemany("INSERT INTO loci(locus) VALUES (?)", [(locus_name(n),) for n in names])
    keys = [r[0] for r in c.execute("SELECT id FROM loci ORDER BY id DESC LIMIT ?", (L,)).fetchall()][::-1]
    keys = np.asarray(keys, dtype=np.int64)
    if T:
        c.executemany("INSERT INTO net VALUES (?,?,?)",
                      zip(np.repeat(keys, T).tolist(), np.tile(np.arange(T), L).tolist(), tables[:, :T].reshape(-1).tolist()))
    if n_t:
        c.executemany("INSERT INTO discrete VALUES (?,?,?)",
                      zip(np.repeat(keys, n_t).tolist(), np.tile(np.asarray(times, dtype=np.int64), L).tolist(),
                          tables[:, T:T + n_t].reshape(-1).tolist()))
    if n_i:
        c.executemany("INSERT INTO interval VALUES (?,?,?,?)",
                      zip(np.repeat(keys, n_i).tolist(), labels * L, tables[:, T + n_t:T + n_t + n_i].reshape(-1).tolist(),
                          tables[:, T + n_t + n_i:T + n_t + 2 * n_i].reshape(-1).tolist()))


BOOTSTRAP_DDL = [
    "CREATE TABLE loci (id INTEGER PRIMARY KEY AUTOINCREMENT, locus TEXT)",
    "CREATE TABLE net_bootstrap (id INT, time INT, mean FLOAT, sd FLOAT, lo FLOAT, hi FLOAT, FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE discrete_bootstrap (id INT, time INT, mean FLOAT, sd FLOAT, lo FLOAT, hi FLOAT, FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE interval_bootstrap (id INT, interval TEXT, mean FLOAT, sd FLOAT, lo FLOAT, hi FLOAT, FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE meta (key TEXT PRIMARY KEY, value TEXT)",
]


def write_bootstrap_db(db_name, names, summary, T, times, intervals, replicates, seed, level, method=None):
    """phylogenetic-informativeness-bootstrap.sqlite, a file of its own beside the main database (which stays byte for
    byte what it is without --bootstrap).  summary [L, 4, T + n_i] = mean, sd, lo, hi per locus (pipeline.bootstrap_tables);
    the --times rows are the net rows at those times.  Loci get the ids 1..L in file order, as in the main database.
    Bulk inserts as in insert_tables.  method: None for the site bootstrap; "parametric" writes the same tables for
    phylogenetic-informativeness-parametric-bootstrap.sqlite (pipeline.parametric_bootstrap_tables) with a `method` row in meta."""
    import numpy as np
    if os.path.exists(db_name):
        os.remove(db_name)
    conn = sqlite3.connect(db_name)
    c = conn.cursor()
    for stmt in BOOTSTRAP_DDL:
        c.execute(stmt)
    L, n_t, n_i = len(names), len(times), len(intervals)
    summary = np.asarray(summary, dtype=np.float64).reshape(L, 4, T + n_i)
    c.executemany("INSERT INTO loci(locus) VALUES (?)", [(locus_name(n),) for n in names])
    keys = np.asarray([r[0] for r in c.execute("SELECT id FROM loci ORDER BY id").fetchall()], dtype=np.int64)

    def stats(block):   # [L, 4, k] -> four flat columns, locus by locus
        return [block[:, j, :].reshape(-1).tolist() for j in range(4)]

    if L and T:
        c.executemany("INSERT INTO net_bootstrap VALUES (?,?,?,?,?,?)",
                      zip(np.repeat(keys, T).tolist(), np.tile(np.arange(T), L).tolist(), *stats(summary[:, :, :T])))
    if L and n_t:
        tt = np.asarray(times, dtype=np.int64)
        c.executemany("INSERT INTO discrete_bootstrap VALUES (?,?,?,?,?,?)",
                      zip(np.repeat(keys, n_t).tolist(), np.tile(tt, L).tolist(), *stats(summary[:, :, tt])))
    if L and n_i:
        labels = ["{0}-{1}".format(a, b) for a, b in intervals]
        c.executemany("INSERT INTO interval_bootstrap VALUES (?,?,?,?,?,?)",
                      zip(np.repeat(keys, n_i).tolist(), labels * L, *stats(summary[:, :, T:])))
    c.executemany("INSERT INTO meta VALUES (?,?)", [("replicates", str(int(replicates))), ("seed", str(int(seed))),
                                                    ("level", repr(float(level)))])
    if method is not None:
        c.execute("INSERT INTO meta VALUES (?,?)", ("method", str(method)))
    conn.commit()
    c.close()
    conn.close()


POSTERIOR_DDL = [
    "CREATE TABLE loci (id INTEGER PRIMARY KEY AUTOINCREMENT, locus TEXT)",
    "CREATE TABLE net_posterior (id INT, time INT, mean FLOAT, sd FLOAT, lo FLOAT, hi FLOAT, FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE discrete_posterior (id INT, time INT, mean FLOAT, sd FLOAT, lo FLOAT, hi FLOAT, FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE interval_posterior (id INT, interval TEXT, mean FLOAT, sd FLOAT, lo FLOAT, hi FLOAT, FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE category (id INT, k INT, rate FLOAT, expected_sites FLOAT, FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE meta (key TEXT PRIMARY KEY, value TEXT)",
]


def write_posterior_db(db_name, names, bands, category_rate, expected_sites, alpha, scale, T, times, intervals, replicates, seed,
                       level):
    """phylogenetic-informativeness-posterior.sqlite (--posterior-pi), a file of its own laid out like the bootstrap file; the main
    database stays byte for byte what it is without the flag.  bands [L, 4, T + n_i] = mean, sd, lo, hi per locus
    (pipeline.posterior_pi_tables): mean and sd are the analytic moments of the locus' PI row under the empirical-Bayes rate
    posterior, lo and hi the quantiles of the `replicates` posterior draws.  category_rate and expected_sites [L, K]: the final
    rate of every gamma category and the expected number of informative sites in it.  meta: replicates, seed, level,
    categories, and alpha_<id> / scale_<id> per locus -- everything is conditional on that fit."""
    import numpy as np
    if os.path.exists(db_name):
        os.remove(db_name)
    conn = sqlite3.connect(db_name)
    c = conn.cursor()
    for stmt in POSTERIOR_DDL:
        c.execute(stmt)
    L, n_t, n_i = len(names), len(times), len(intervals)
    bands = np.asarray(bands, dtype=np.float64).reshape(L, 4, T + n_i)
    category_rate = np.asarray(category_rate, dtype=np.float64).reshape(L, -1)
    expected_sites = np.asarray(expected_sites, dtype=np.float64).reshape(L, -1)
    K = category_rate.shape[1]
    c.executemany("INSERT INTO loci(locus) VALUES (?)", [(locus_name(n),) for n in names])
    keys = np.asarray([r[0] for r in c.execute("SELECT id FROM loci ORDER BY id").fetchall()], dtype=np.int64)

    def stats(block):   # [L, 4, k] -> four flat columns, locus by locus
        return [block[:, j, :].reshape(-1).tolist() for j in range(4)]

    if L and T:
        c.executemany("INSERT INTO net_posterior VALUES (?,?,?,?,?,?)",
                      zip(np.repeat(keys, T).tolist(), np.tile(np.arange(T), L).tolist(), *stats(bands[:, :, :T])))
    if L and n_t:
        tt = np.asarray(times, dtype=np.int64)
        c.executemany("INSERT INTO discrete_posterior VALUES (?,?,?,?,?,?)",
                      zip(np.repeat(keys, n_t).tolist(), np.tile(tt, L).tolist(), *stats(bands[:, :, tt])))
    if L and n_i:
        labels = ["{0}-{1}".format(a, b) for a, b in intervals]
        c.executemany("INSERT INTO interval_posterior VALUES (?,?,?,?,?,?)",
                      zip(np.repeat(keys, n_i).tolist(), labels * L, *stats(bands[:, :, T:])))
    if L and K:
        c.executemany("INSERT INTO category VALUES (?,?,?,?)",
                      zip(np.repeat(keys, K).tolist(), np.tile(np.arange(K), L).tolist(), category_rate.reshape(-1).tolist(),
                          expected_sites.reshape(-1).tolist()))
    c.executemany("INSERT INTO meta VALUES (?,?)", [("replicates", str(int(replicates))), ("seed", str(int(seed))),
                                                    ("level", repr(float(level))), ("categories", str(int(K)))])
    c.executemany("INSERT INTO meta VALUES (?,?)",
                  [("alpha_%d" % k, repr(float(a))) for k, a in zip(keys.tolist(), np.asarray(alpha, dtype=np.float64).reshape(-1))] +
                  [("scale_%d" % k, repr(float(s))) for k, s in zip(keys.tolist(), np.asarray(scale, dtype=np.float64).reshape(-1))])
    conn.commit()
    c.close()
    conn.close()


QUARTET_DDL = [
    "CREATE TABLE loci (id INTEGER PRIMARY KEY AUTOINCREMENT, locus TEXT)",
    "CREATE TABLE quartet (id INT, quartet TEXT, tip FLOAT, internode FLOAT, signal FLOAT, noise FLOAT, p_correct FLOAT, "
    "p_incorrect FLOAT, p_polytomy FLOAT, FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE meta (key TEXT PRIMARY KEY, value TEXT)",
]


def write_quartet_db(db_name, names, rows, labels, quartets, model):
    """phylogenetic-informativeness-quartets.sqlite, a file of its own beside the main database (which stays byte for byte
    what it is without --quartets).  rows [L, n_q, 8] from pipeline.quartet_tables; labels: the quartets "T:to" as typed;
    quartets [n_q, 2] their values.  signal and noise are the expected numbers of signal sites (Y) and of noise sites for
    one wrong topology (X).  Loci get the ids 1..L in file order, as in the main database."""
    import numpy as np
    if os.path.exists(db_name):
        os.remove(db_name)
    conn = sqlite3.connect(db_name)
    c = conn.cursor()
    for stmt in QUARTET_DDL:
        c.execute(stmt)
    L, n_q = len(names), len(labels)
    rows = np.asarray(rows, dtype=np.float64).reshape(L, n_q, 8)
    quartets = np.asarray(quartets, dtype=np.float64).reshape(n_q, 2)
    c.executemany("INSERT INTO loci(locus) VALUES (?)", [(locus_name(n),) for n in names])
    keys = np.asarray([r[0] for r in c.execute("SELECT id FROM loci ORDER BY id").fetchall()], dtype=np.int64)
    if L and n_q:
        c.executemany("INSERT INTO quartet VALUES (?,?,?,?,?,?,?,?,?)",
                      zip(np.repeat(keys, n_q).tolist(), list(labels) * L, np.tile(quartets[:, 0], L).tolist(),
                          np.tile(quartets[:, 1], L).tolist(), rows[:, :, 0].reshape(-1).tolist(), rows[:, :, 1].reshape(-1).tolist(),
                          rows[:, :, 5].reshape(-1).tolist(), rows[:, :, 6].reshape(-1).tolist(), rows[:, :, 7].reshape(-1).tolist()))
    c.executemany("INSERT INTO meta VALUES (?,?)", [("quartets", ",".join(labels)), ("model", str(model)),
                                                    ("approximation", "bivariate normal with continuity correction")])
    conn.commit()
    c.close()
    conn.close()


def add_quartet_exact_table(db_name, rows, labels, window_cap, unequal=False):
    """--exact-quartets: the table quartet_exact and its `meta` rows, added to a quartet database that write_quartet_db or
    write_unequal_quartet_db (unequal=True) has just written.  rows [L, n_q, 6] from pipeline.exact_quartet_tables
    (p_correct, p_ac, p_ad, p_polytomy, window, tail_bound).  The equal-tip file stores p_incorrect = p_ac + p_ad, the
    unequal one p_ac and p_ad; a pair that was not computed (window 0) has NULL probabilities."""
    import numpy as np
    conn = sqlite3.connect(db_name)
    c = conn.cursor()
    wrong = "p_ac FLOAT, p_ad FLOAT" if unequal else "p_incorrect FLOAT"
    c.execute("CREATE TABLE quartet_exact (id INT, quartet TEXT, p_correct FLOAT, " + wrong + ", p_polytomy FLOAT, window INT, "
              "tail_bound FLOAT, FOREIGN KEY(id) REFERENCES loci(id))")
    keys = [r[0] for r in c.execute("SELECT id FROM loci ORDER BY id").fetchall()]
    L, n_q = len(keys), len(labels)
    rows = np.asarray(rows, dtype=np.float64).reshape(L, n_q, 6)
    out = []
    for l in range(L):
        for q in range(n_q):
            pc, p1, p2, rest, window, bound = rows[l, q].tolist()
            if window == 0:
                probs = (None,) * (4 if unequal else 3)
            else:
                probs = (pc, p1, p2, rest) if unequal else (pc, p1 + p2, rest)
            out.append((keys[l], labels[q]) + probs + (int(window), bound))
    c.executemany("INSERT INTO quartet_exact VALUES (" + ",".join("?" * (8 if unequal else 7)) + ")", out)
    c.executemany("INSERT INTO meta VALUES (?,?)",
                  [("exact", "characteristic function of the counts on a window x window torus: exact to tail_bound and rounding"),
                   ("exact_window_cap", str(int(window_cap))), ("exact_tail_tolerance", "1e-12")])
    conn.commit()
    c.close()
    conn.close()


UNEQUAL_QUARTET_DDL = [
    "CREATE TABLE loci (id INTEGER PRIMARY KEY AUTOINCREMENT, locus TEXT)",
    "CREATE TABLE quartet (id INT, quartet TEXT, tip_a FLOAT, tip_b FLOAT, tip_c FLOAT, tip_d FLOAT, internode FLOAT, "
    "signal FLOAT, noise_ac FLOAT, noise_ad FLOAT, p_correct FLOAT, p_ac FLOAT, p_ad FLOAT, p_polytomy FLOAT, "
    "FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE clade (quartet TEXT, ntaxa INT, taxa TEXT)",
    "CREATE TABLE meta (key TEXT PRIMARY KEY, value TEXT)",
]


def write_unequal_quartet_db(db_name, names, rows, labels, quartets, model, clades=()):
    """phylogenetic-informativeness-unequal-quartets.sqlite, a third file of its own (every other output stays byte for byte
    what it is without --unequal-quartets / --tree-quartets).  rows [L, n_q, 13] from pipeline.unequal_quartet_tables;
    labels: the typed quartets "Ta/Tb/Tc/Td:to" as typed, then node1, node2, ... for the tree's; quartets [n_q, 5] their
    values.  signal, noise_ac and noise_ad are the expected numbers of sites of the patterns iijj, ijij and ijji.  clades:
    (label, leaf names) per tree quartet: the clade below the internode, comma-joined.  Loci get the ids 1..L in file order."""
    import numpy as np
    if os.path.exists(db_name):
        os.remove(db_name)
    conn = sqlite3.connect(db_name)
    c = conn.cursor()
    for stmt in UNEQUAL_QUARTET_DDL:
        c.execute(stmt)
    L, n_q = len(names), len(labels)
    rows = np.asarray(rows, dtype=np.float64).reshape(L, n_q, 13)
    quartets = np.asarray(quartets, dtype=np.float64).reshape(n_q, 5)
    c.executemany("INSERT INTO loci(locus) VALUES (?)", [(locus_name(n),) for n in names])
    keys = np.asarray([r[0] for r in c.execute("SELECT id FROM loci ORDER BY id").fetchall()], dtype=np.int64)
    if L and n_q:
        c.executemany("INSERT INTO quartet VALUES (?,?,?,?,?,?,?,?,?,?,?,?,?,?)",
                      zip(np.repeat(keys, n_q).tolist(), list(labels) * L, *[np.tile(quartets[:, k], L).tolist() for k in range(5)],
                          *[rows[:, :, k].reshape(-1).tolist() for k in (0, 1, 2, 9, 10, 11, 12)]))
    c.executemany("INSERT INTO clade VALUES (?,?,?)", [(label, len(taxa), ",".join(taxa)) for label, taxa in clades])
    c.executemany("INSERT INTO meta VALUES (?,?)", [("quartets", ",".join(labels)), ("model", str(model)),
                                                    ("approximation", "bivariate normal with continuity correction"),
                                                    ("tree_quartets", "nearest tip on each side of the internode")])
    conn.commit()
    c.close()
    conn.close()


CONCORDANCE_RULE_VERSION = 1
_CONCORDANCE_COLUMNS = ("pooled_c INTEGER, pooled_1 INTEGER, pooled_2 INTEGER, pooled_cf FLOAT, pooled_df1 FLOAT, pooled_df2 FLOAT, "
                        "near_c INTEGER, near_1 INTEGER, near_2 INTEGER, sCF FLOAT, sDF1 FLOAT, sDF2 FLOAT, sN FLOAT, "
                        "n_decisive INTEGER, n_quartets INTEGER")
CONCORDANCE_DDL = [
    "CREATE TABLE loci (id INTEGER PRIMARY KEY AUTOINCREMENT, locus TEXT)",
    "CREATE TABLE internode (label TEXT PRIMARY KEY, size_a INT, size_b INT, size_c INT, size_d INT, n_all_quartets INTEGER, "
    "n_quartets INT, enumerated INT)",
    "CREATE TABLE clade (quartet TEXT, ntaxa INT, taxa TEXT, taxa_a TEXT, taxa_b TEXT, taxa_c TEXT, taxa_d TEXT, nearest TEXT)",
    "CREATE TABLE concordance (id INT, internode TEXT, " + _CONCORDANCE_COLUMNS + ", FOREIGN KEY(id) REFERENCES loci(id))",
    "CREATE TABLE concordance_all (internode TEXT, " + _CONCORDANCE_COLUMNS + ")",
    "CREATE TABLE meta (key TEXT PRIMARY KEY, value TEXT)",
]


def _concordance_values(row):
    """The 15 stored values of one row of 12: counts as integers, the pooled fractions (NULL when no quartet is decisive), NaN as
    NULL."""
    import math
    pooled = [int(v) for v in row[:3]]
    total = sum(pooled)
    means = [None if math.isnan(v) else float(v) for v in row[6:10]]
    return (pooled + [p / total if total else None for p in pooled] + [int(v) for v in row[3:6]] + means
            + [int(row[10]), int(row[11])])


def write_concordance_db(db_name, names, rows, all_rows, groups, sets, quartets, seed, clades):
    """phylogenetic-informativeness-concordance.sqlite, a file of its own (every other output stays byte for byte what it is
    without --site-concordance).  rows [L, n_nodes, 12] from pipeline.concordance_tables; all_rows [n_nodes, 12]: the same for
    all loci analysed as one alignment; groups: compute.tree_concordance_groups' entries; sets: compute.concordance_sets'
    tables; clades: (label, leaf names) per internode as the unequal-quartets file has them (at a polytomy the clade holds
    more than groups A and B).  `clade` carries them with the four groups' taxa and the nearest-tip quartet, comma-joined.
    Loci get the ids 1..L in file order."""
    import numpy as np
    if os.path.exists(db_name):
        os.remove(db_name)
    conn = sqlite3.connect(db_name)
    c = conn.cursor()
    for stmt in CONCORDANCE_DDL:
        c.execute(stmt)
    L, n_nodes = len(names), len(groups)
    rows = np.asarray(rows, dtype=np.float64).reshape(L, n_nodes, 12)
    all_rows = np.asarray(all_rows, dtype=np.float64).reshape(n_nodes, 12)
    c.executemany("INSERT INTO loci(locus) VALUES (?)", [(locus_name(n),) for n in names])
    keys = [r[0] for r in c.execute("SELECT id FROM loci ORDER BY id").fetchall()]
    node_sets = [int(v) for v in sets["node_sets"]]
    for i, (label, A, B, C, D, nearest) in enumerate(groups):
        total = len(A) * len(B) * len(C) * len(D)
        c.execute("INSERT INTO internode VALUES (?,?,?,?,?,?,?,?)",
                  (label, len(A), len(B), len(C), len(D), total, node_sets[i + 1] - node_sets[i] - 2, int(bool(sets["enumerated"][i]))))
        clade = clades[i][1]
        c.execute("INSERT INTO clade VALUES (?,?,?,?,?,?,?,?)",
                  (label, len(clade), ",".join(clade), ",".join(A), ",".join(B), ",".join(C), ",".join(D), ",".join(nearest)))
    c.executemany("INSERT INTO concordance VALUES (" + ",".join("?" * 17) + ")",
                  [[keys[l], groups[i][0]] + _concordance_values(rows[l, i]) for l in range(L) for i in range(n_nodes)])
    c.executemany("INSERT INTO concordance_all VALUES (" + ",".join("?" * 16) + ")",
                  [[groups[i][0]] + _concordance_values(all_rows[i]) for i in range(n_nodes)])
    c.executemany("INSERT INTO meta VALUES (?,?)", [("seed", str(seed)), ("quartets_per_internode", str(quartets)),
                                                    ("rule_version", str(CONCORDANCE_RULE_VERSION)),
                                                    ("rule", "cells of exactly one base; xxyy, xyxy, xyyx with x != y")])
    conn.commit()
    c.close()
    conn.close()


LOCUS_SET_SUMS = {False: ("Y", "X", "Yy", "Xx", "XY"), True: ("Y", "X1", "X2", "Yy", "X1x1", "X2x2", "YX1", "YX2", "X1X2")}


def add_locus_set_tables(db_name, rows, order, labels, target, order_rule, max_k, unequal=False, exact=None, window_cap=None):
    """--locus-sets: the accumulation curves over an ordered list of loci, added to a quartet database
    that write_quartet_db or write_unequal_quartet_db (unequal=True) has just written.  rows [n_q, K, 8 or 13] from
    pipeline.locus_set_tables and order [n_q, K] (indices into the file's loci, in file order) -> the table locus_set: per
    quartet and k the locus added at step k (`id`), the sums of the set of the first k loci and its normal-approximation
    probabilities.  locus_set_summary: per quartet the target, the smallest k whose p_correct reaches it (NULL if none does)
    and p_correct of the whole list.  exact [n_q, K, 6] from pipeline.exact_locus_set_tables (--exact-quartets) -> the table
    locus_set_exact (a prefix that was not computed has NULL probabilities and window 0) and the column k_needed_exact, NULL
    when no computed prefix reaches the target.  meta: the order rule, the maximum, the target and the cap."""
    import numpy as np
    conn = sqlite3.connect(db_name)
    c = conn.cursor()
    sums = LOCUS_SET_SUMS[bool(unequal)]
    width = len(sums) + (4 if unequal else 3)
    wrong = "p_ac FLOAT, p_ad FLOAT" if unequal else "p_incorrect FLOAT"
    c.execute("CREATE TABLE locus_set (quartet TEXT, k INT, id INT, " + ", ".join(s + " FLOAT" for s in sums) + ", p_correct FLOAT, "
              + wrong + ", p_polytomy FLOAT, FOREIGN KEY(id) REFERENCES loci(id))")
    c.execute("CREATE TABLE locus_set_summary (quartet TEXT, target FLOAT, k_needed INT, p_correct_all FLOAT"
              + (", k_needed_exact INT" if exact is not None else "") + ")")
    keys = [r[0] for r in c.execute("SELECT id FROM loci ORDER BY id").fetchall()]
    order = np.asarray(order, dtype=np.int64)
    n_q, K = len(labels), order.shape[1] if order.ndim == 2 else 0
    rows = np.asarray(rows, dtype=np.float64).reshape(n_q, K, width)
    p_col = len(sums)

    def first_reaching(p):   # the smallest k (from 1) with p >= target; NaN never is
        hit = np.flatnonzero(p >= target)
        return int(hit[0]) + 1 if hit.size else None

    out, summary = [], []
    for q in range(n_q):
        for k in range(K):
            out.append((labels[q], k + 1, keys[int(order[q, k])]) + tuple(rows[q, k].tolist()))
        row = (labels[q], float(target), first_reaching(rows[q, :, p_col]), float(rows[q, K - 1, p_col]) if K else None)
        if exact is not None:
            with np.errstate(invalid="ignore"):
                row += (first_reaching(np.asarray(exact, dtype=np.float64).reshape(n_q, K, 6)[q, :, 0]),)
        summary.append(row)
    c.executemany("INSERT INTO locus_set VALUES (" + ",".join("?" * (3 + width)) + ")", out)
    c.executemany("INSERT INTO locus_set_summary VALUES (" + ",".join("?" * (5 if exact is not None else 4)) + ")", summary)
    meta = [("locus_sets_order", str(order_rule)), ("locus_sets_max", "all" if max_k is None else str(int(max_k))),
            ("locus_sets_target", repr(float(target)))]
    if exact is not None:
        exact = np.asarray(exact, dtype=np.float64).reshape(n_q, K, 6)
        c.execute("CREATE TABLE locus_set_exact (quartet TEXT, k INT, p_correct FLOAT, " + wrong + ", p_polytomy FLOAT, window INT, "
                  "tail_bound FLOAT)")
        out = []
        for q in range(n_q):
            for k in range(K):
                pc, p1, p2, rest, window, bound = exact[q, k].tolist()
                if window == 0:
                    probs = (None,) * (4 if unequal else 3)
                else:
                    probs = (pc, p1, p2, rest) if unequal else (pc, p1 + p2, rest)
                out.append((labels[q], k + 1) + probs + (int(window), bound))
        c.executemany("INSERT INTO locus_set_exact VALUES (" + ",".join("?" * (8 if unequal else 7)) + ")", out)
        meta.append(("locus_sets_window_cap", str(int(window_cap))))
    c.executemany("INSERT INTO meta VALUES (?,?)", meta)
    conn.commit()
    c.close()
    conn.close()
