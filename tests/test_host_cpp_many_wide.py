"""Lock-step POA builds (`poasta_align_amd align-many`) of reads longer than one strip of the packed forward pass: the exact
multi-graph batch under align_multi is created with POA_CFG_WIDE_QUERIES as soon as a read exceeds 1023 symbols.  Every output
is byte-identical to the oracle's sequential build of that file and to what `poasta_align_amd align` writes for it alone."""
import os
import subprocess

import numpy as np
import pytest

from poasta_amd import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALIGN_DRIVER = os.path.join(ROOT, "poasta_amd", "poasta_align_amd")
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def driver():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "poasta_amd", "csrc")], stdout=subprocess.DEVNULL)
    assert os.path.exists(ALIGN_DRIVER)
    return ALIGN_DRIVER


def _indels(rng, seq, n):
    """n single indels of one to three bases at random places."""
    seq = list(seq)
    for _ in range(n):
        at, k = int(rng.integers(10, len(seq) - 10)), int(rng.integers(1, 4))
        if rng.random() < 0.5:
            del seq[at:at + k]
        else:
            seq[at:at] = [int(b) for b in rng.choice(ACGT, k)]
    return np.array(seq, np.uint8)


def _builds(tmp_path):
    """Two builds, of three and of four reads of 1050 - 1250 bp: a common sequence per build, every read a window of it with 1 %
    substitutions and a few indels.  Seeded; written to tmp_path."""
    rng = np.random.default_rng(61)
    files, outs = [], []
    for k, n_reads in enumerate((3, 4)):
        common = rng.choice(ACGT, 1260)
        reads = []
        for r in range(n_reads):
            length = (1050, 1250, 1140, 1199)[(r + k) % 4]
            a = int(rng.integers(0, len(common) - length + 1)) if r else 0
            read = _indels(rng, W.mutate(rng, common[a:a + length + 6], 0.01, 0.0, 0.0), 4)[:length]
            assert 1050 <= len(read) <= 1250
            reads.append(read)
        path = os.path.join(str(tmp_path), "reads%d.fa" % k)
        with open(path, "w") as f:
            for r, read in enumerate(reads):
                f.write(">build%d_read%d\n%s\n" % (k, r, read.tobytes().decode()))
        files.append(path)
        outs.append(os.path.join(str(tmp_path), "out%d.fa" % k))
    lst = os.path.join(str(tmp_path), "list.tsv")
    with open(lst, "w") as f:
        for path, out in zip(files, outs):
            f.write(path + "\t" + out + "\n")
    return lst, files, outs


@pytest.mark.gpu
def test_gpu_lock_step_builds_of_long_reads_equal_oracle_and_align(driver, oracle, tmp_path):
    lst, files, outs = _builds(tmp_path)
    for path in files:
        lens = [len(s) for _, s in oracle.read_fasta(path)]
        assert len(lens) in (3, 4) and min(lens) >= 1050 and max(lens) <= 1250, lens
    opts = ["-H", "mingap"]
    r = subprocess.run([driver, "align-many", *opts, lst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for path, out in zip(files, outs):
        got = open(out).read()
        g, _ = oracle.sequential_poa(oracle.read_fasta(path), oracle.Costs(4, 6, 2), heuristic=oracle.H_MINGAP)
        assert got == g.to_fasta(), (path, "oracle")
        alone = subprocess.check_output([driver, "align", *opts, path], stderr=subprocess.DEVNULL).decode()
        assert got == alone, (path, "align")
