// The block lease of the streaming interface (rvtests_amd/csrc/block_pool.h) with fake allocate / free callbacks: every way
// out of a submission returns its block to the pool exactly once, and a released lease returns nothing.  Host code only; built
// with the address and undefined-behaviour sanitizers (tests/test_block_pool_cpu.py), so a block freed twice, kept or lost shows
// as a report as well as a failed check.
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I rvtests_amd/csrc tools/block_lease_check.cpp
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "block_pool.h"

using rvt::BlockLease;
using rvt::BlockPool;

static int g_allocs = 0, g_frees = 0, g_failed = 0;
static bool g_alloc_fails = false;
static double* fake_alloc(size_t bytes) {
  if (g_alloc_fails) return nullptr;
  ++g_allocs;
  return static_cast<double*>(std::malloc(bytes));  // (really allocated: a double free or a leak is the sanitizer's to find)
}
static void fake_free(double* p) {
  ++g_frees;
  std::free(p);
}
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);         \
      ++g_failed;                                                     \
    }                                                                 \
  } while (0)

struct Queued {  // what a submitted gene keeps of its block (rvt_ctx::Pending)
  double* ptr = nullptr;
  size_t bytes = 0;
};

// a submission in the shape of the engine's: lease, three steps that may fail, enqueue.  fail_at: 0 none, 1 .. 3 the step.
static int submit(BlockPool& pool, size_t need, bool bounded, int fail_at, std::vector<Queued>& queue) {
  BlockLease blk(pool, need, bounded, fake_alloc);
  if (!blk) return -3;
  if (fail_at == 1) return -1;  // work space
  for (int step = 2; step <= 3; ++step)
    if (fail_at == step) return -step;  // copy, consolidation
  Queued q;
  q.ptr = blk.release(&q.bytes);
  queue.push_back(q);
  return 0;
}

int main() {
  BlockPool pool;
  std::vector<Queued> queue;
  // every early return gives the block back once: the pool grows by one at the first failure and stays at one after it
  for (int fail_at = 1; fail_at <= 3; ++fail_at) {
    CHECK(submit(pool, 4096, true, fail_at, queue) == -fail_at);
    CHECK(pool.free_blocks.size() == 1 && queue.empty());
    CHECK(pool.free_blocks[0].bytes == 4096);
  }
  CHECK(g_allocs == 1);
  // a released lease returns nothing: the block is the queue's
  CHECK(submit(pool, 2048, true, 0, queue) == 0);
  CHECK(pool.free_blocks.empty() && queue.size() == 1);
  CHECK(queue[0].bytes == 4096);  // (the capacity, not the 2048 bytes asked for)
  CHECK(g_allocs == 1);
  // the collect path hands it back with that capacity
  pool.give(queue[0].bytes, queue[0].ptr);
  queue.clear();
  CHECK(pool.free_blocks.size() == 1 && pool.free_blocks[0].bytes == 4096);
  // more than four times the need: left alone, a fresh block is made; both return at the failure
  {
    BlockLease small(pool, 512, true, fake_alloc);
    CHECK(small && small.fresh() && small.bytes() == 512 && g_allocs == 2);
    BlockLease big(pool, 512, false, fake_alloc);
    CHECK(big && !big.fresh() && big.bytes() == 4096);
    // moved leases: the block goes back once, from where it ended up
    BlockLease moved(std::move(small));
    CHECK(!small && moved && moved.bytes() == 512);
    std::vector<BlockLease> many;
    many.push_back(std::move(big));
    many.push_back(std::move(moved));
    CHECK(pool.free_blocks.empty());
    BlockLease target(pool, 64, true, fake_alloc);
    CHECK(target.fresh() && g_allocs == 3);
    target = std::move(many[1]);  // the 64-byte block goes back here, the 512-byte one at the end of the scope
    CHECK(pool.free_blocks.size() == 1 && pool.free_blocks[0].bytes == 64);
  }
  CHECK(pool.free_blocks.size() == 3 && pool.bytes() == 64 + 4096 + 512);
  // an allocation that fails: an empty lease, nothing to return
  g_alloc_fails = true;
  CHECK(submit(pool, 1 << 20, true, 0, queue) == -3);
  g_alloc_fails = false;
  CHECK(pool.free_blocks.size() == 3 && queue.empty());
  // the bounded trim, then everything: each block freed once (the sanitizer sees a second free or a forgotten block)
  pool.trim(4096 + 64, 8, fake_free);
  CHECK(pool.free_blocks.size() == 2 && g_frees == 1);
  pool.clear(fake_free);
  CHECK(pool.free_blocks.empty() && g_frees == 3 && g_allocs == 3);
  if (g_failed) return 1;
  std::puts("block lease: ok");
  return 0;
}
