"""Lock-step POA builds (`poasta_align_amd align-many`): many graphs built read by read, one read of every build per round through
one exact multi-graph run (aligner::PoastaAligner::align_multi over poa_multi_*_exact), the graph updates between rounds.
Every output is byte-identical to the oracle's sequential build of that file and to what `poasta_align_amd align` writes for
it alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN_DRIVER = os.path.join(ROOT, "poasta_amd", "poasta_align_amd")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "poasta_amd", "csrc")], stdout=subprocess.DEVNULL)
    assert os.path.exists(ALIGN_DRIVER)
    return ALIGN_DRIVER


def _list(tmp_path, name="list.tsv"):
    """Three builds with different read counts (so builds drop out), the third seeded with an MSA."""
    builds = [("test_from_abpoa.fa", None), ("test2_from_abpoa.fa", None), ("small_test.query.fa", "small_test.input.fa")]
    outs = [os.path.join(str(tmp_path), "out%d.fa" % k) for k in range(len(builds))]
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        for (reads, seed), out in zip(builds, outs):
            f.write("\t".join([os.path.join(GOLD, reads), out] + ([os.path.join(GOLD, seed)] if seed else [])) + "\n")
    return path, builds, outs


def _oracle_msa(oracle, reads, seed, heuristic):
    g = oracle.OracleGraph.from_fasta_msa(oracle.read_fasta(os.path.join(GOLD, seed))) if seed else None
    g, _ = oracle.sequential_poa(oracle.read_fasta(os.path.join(GOLD, reads)), oracle.Costs(4, 6, 2), heuristic=heuristic, graph=g)
    return g.to_fasta()


@pytest.mark.gpu
@pytest.mark.parametrize("heur", ["mingap", "dijkstra"])
def test_gpu_lock_step_builds_equal_oracle_and_align(driver, oracle, tmp_path, heur):
    path, builds, outs = _list(tmp_path)
    counts = [len(oracle.read_fasta(os.path.join(GOLD, reads))) for reads, _ in builds]
    assert len(set(counts)) > 1, "the builds must drop out at different rounds"
    timing = os.path.join(str(tmp_path), "timing.tsv")
    opts = ["-H", heur]
    r = subprocess.run([driver, "align-many", *opts, "--timing", timing, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for (reads, seed), out in zip(builds, outs):
        got = open(out).read()
        assert got == _oracle_msa(oracle, reads, seed, oracle.H_MINGAP if heur == "mingap" else oracle.H_DIJKSTRA), (reads, "oracle")
        alone = subprocess.check_output([driver, "align", *opts, *(["-I", os.path.join(GOLD, seed)] if seed else []), os.path.join(GOLD, reads)],
                                        stderr=subprocess.DEVNULL).decode()
        assert got == alone, (reads, "align")
    # one line per round that aligned something; the number of graphs falls as builds run out of reads
    rows = [l.split("\t") for l in open(timing).read().splitlines()[1:]]
    n_graphs = [int(f[1]) for f in rows]
    # round r aligns read r of every build that has one; an unseeded build spends read 0 on seeding its graph
    expect = [sum(1 for c, (_, seed) in zip(counts, builds) if (0 if seed else 1) <= r < c) for r in range(max(counts))]
    assert n_graphs == [e for e in expect if e] and max(n_graphs) >= 2 and n_graphs[-1] == 1


def test_lock_step_builds_refuse_two_piece_and_ends_free(driver, tmp_path):
    """Refused before a read is aligned (no device needed): exit status 1 with the PoastaError text of align_multi."""
    path, _, outs = _list(tmp_path)
    for opts, word in ((["-g", "6,24", "-e", "2,1"], "two-piece"), (["-m", "ends-free"], "ends-free"), (["-m", "semi-global"], "ends-free"),
                       (["--mode", "dense"], "Mode::Exact")):
        r = subprocess.run([driver, "align-many", *opts, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1, (opts, r.returncode)
        assert b"align_multi" in r.stderr and word.encode() in r.stderr, (opts, r.stderr)
        assert not any(os.path.exists(o) for o in outs)
    r = subprocess.run([driver, "align-many", "-o", "x.fa", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"name them in the list" in r.stderr
