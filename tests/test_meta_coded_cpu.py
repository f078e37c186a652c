"""CPU: `--meta dominant` / `--meta recessive` in the host adapters' registry (src/ModelManager.cpp:211-226): each name makes
a score model and a covariance model, in that order, with the reference's file names.  Without a device nothing is computed:
the covariance sections hold their header only and the score sections the callers' site counters with NA statistics — never
a CPU result."""
import numpy as np
import pytest

from test_host_driver import _case, _ensure_driver, run_driver_meta

COV_HEADER = ["CHROM", "START_POS", "END_POS", "NUM_MARKER", "MARKER_POS", "COV"]


def sections_of(lines):
    sec, cur = {}, None
    for ln in lines:
        if ln.startswith("== "):
            cur = ln[3:]
            sec[cur] = []
        else:
            sec[cur].append(ln.split("\t"))
    return sec


def _sites(tmp_path, genes):
    sites = str(tmp_path / "sites.txt")
    with open(sites, "w") as f:
        k = 0
        for G, af in genes:
            for j in range(G.shape[1]):
                f.write("1 %d\n" % (100 + 10 * k))
                k += 1
    return sites, k


@pytest.mark.parametrize("name,Name", [("dominant", "MetaDominant"), ("recessive", "MetaRecessive")])
def test_coded_meta_registry_without_gpu(tmp_path, name, Name):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    _ensure_driver()
    path, genes, X, y, res, v = _case(tmp_path)
    sites, V = _sites(tmp_path, genes)
    rc, lines, err = run_driver_meta(path, "%s[windowSize=200]" % name, sites)
    assert rc == 0, err
    sec = sections_of(lines)
    assert list(sec) == ["out.%s.assoc" % Name, "out.%sCov.assoc" % Name]
    cov = sec["out.%sCov.assoc" % Name]
    assert cov[0] == COV_HEADER
    assert len(cov) == 1                              # no device => no rows, never a CPU result
    score = sec["out.%s.assoc" % Name]
    assert score[0][-4:] == ["U_STAT", "SQRT_V_STAT", "ALT_EFFSIZE", "PVALUE"]
    assert len(score) == 1 + V                        # the sites' counters, as MetaScore prints them ...
    assert all(row[-4:] == ["NA"] * 4 for row in score[1:])   # ... and no statistic


def test_coded_names_next_to_the_additive_ones_and_unknown_names(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu test")
    _ensure_driver()
    path, genes, X, y, res, v = _case(tmp_path)
    sites, V = _sites(tmp_path, genes)
    rc, lines, err = run_driver_meta(path, "score,cov[windowSize=200],recessive,dominant[windowSize=300]", sites)
    assert rc == 0, err
    assert list(sections_of(lines)) == ["out.MetaScore.assoc", "out.MetaCov.assoc", "out.MetaRecessive.assoc",
                                        "out.MetaRecessiveCov.assoc", "out.MetaDominant.assoc", "out.MetaDominantCov.assoc"]
    rc, lines, err = run_driver_meta(path, "nosuch", sites)
    assert rc == 1 and "Unknown model name: nosuch" in err
    rc, lines, err = run_driver_meta(path, "dominantexact", sites)
    assert rc == 1 and "Unknown model name: dominantexact" in err


RECODER_PROGRAM = r'''
// drives ColumnRecoder — the coded models' own put() / ready(), with this program's callbacks in place of the two device calls —
// over rings of several sizes: every column uploaded raw must be recoded exactly once, in runs of consecutive columns of at
// most kMaxPending, before the "device call" that reads it; a failed upload leaves nothing pending for its column, a failed
// recoding is not repeated
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ModelFitterGpu.h"
using rvt_host::ColumnRecoder;
static std::vector<int> state;  // per physical column: 0 empty, 1 raw, 2 recoded
static int recodings = 0, failUpload = -1, failRecode = -1, calls = 0;
static int upload(int c) {
  if (++calls == failUpload) return -1;
  if (c < 0 || c >= (int)state.size()) return -1;
  state[c] = 1;
  return 0;
}
static int recode(int start, int n) {
  if (n < 1 || n > ColumnRecoder::kMaxPending || start < 0 || start + n > (int)state.size()) std::abort();
  for (int k = 0; k < n; ++k) {
    if (state[start + k] != 1) std::abort();  // not uploaded, or recoded twice
    state[start + k] = 2;
  }
  if (++recodings == failRecode) return -1;
  return 0;
}
int main() {
  for (int cap : {2, 16, 33, 64, 1000}) {
    state.assign(cap, 0);
    ColumnRecoder rec;
    int head = 0, size = 0;
    unsigned long long x = 88172645463325252ull;
    for (int site = 0; site < 5000; ++site) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      if (size == cap || x % 97 == 0) {  // a flush: the device reads every column in use
        if (rec.ready(recode)) return 1;
        for (int k = 0; k < size; ++k)
          if (state[(head + k) % cap] != 2) return 2;
        const int drop = size ? 1 + (int)(x % size) : 0;
        for (int k = 0; k < drop; ++k) state[(head + k) % cap] = 0;
        head = (head + drop) % cap, size -= drop;
      }
      if (rec.put((head + size) % cap, upload, recode)) return 3;
      ++size;
      if (rec.pending() >= ColumnRecoder::kMaxPending) return 4;
    }
    if (rec.ready(recode) || rec.pending()) return 5;
  }
  {  // a failed upload: reported, its column does not join the run; a failed recoding: reported once, nothing stays pending
    state.assign(64, 0);
    ColumnRecoder rec;
    calls = 0, failUpload = 3;
    if (rec.put(0, upload, recode) || rec.put(1, upload, recode)) return 6;
    if (rec.put(2, upload, recode) != -1 || rec.pending() != 2) return 7;
    failUpload = -1;
    failRecode = recodings + 1;
    if (rec.ready(recode) != -1 || rec.pending() != 0) return 8;
    failRecode = -1;
    if (rec.ready(recode) != 0) return 9;
  }
  std::printf("ok %d recodings\n", recodings);
  return 0;
}
'''


def test_column_recoder_under_sanitizers(tmp_path):
    """The coded models' host-side bookkeeping (ColumnRecoder, as the adapters call it) in a stand-alone program built with
    -fsanitize=address,undefined (CPU only; no device, nothing of it is loaded into Python)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "column_recoder.cpp"
    src.write_text(RECODER_PROGRAM)
    exe = tmp_path / "column_recoder"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(root, "rvtests_amd", "csrc", "host"), str(src), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    assert p.stdout.startswith("ok ")
