// rvtests_amd — the free lists of the streaming interface's device blocks: which free block a gene gets, how many are kept,
// and a move-only lease that cannot lose one.  Plain C++ with no device call in it: allocation and release are the caller's
// callbacks (rvt_stream.hip gives hipMalloc / hipFree; hostcheck.cpp and tools/block_lease_check.cpp give fakes).
#pragma once
#include <cstddef>
#include <utility>
#include <vector>

namespace rvt {

struct BlockPool {
  struct Entry {
    size_t bytes;  // the block's CAPACITY, whatever the gene that used it last needed
    double* ptr;
  };
  std::vector<Entry> free_blocks;

  // Best fit: the smallest free block of at least `need` bytes, the first of equals; {0, nullptr} when none fits.  bounded
  // (packed blocks): a block of more than 4 x need is left alone — a gene of three rows must not tie up a block of ninety-six.
  Entry take(size_t need, bool bounded) {
    int best = -1;
    for (int i = 0; i < (int)free_blocks.size(); ++i) {
      const size_t b = free_blocks[i].bytes;
      if (b >= need && (!bounded || b <= 4 * need) && (best < 0 || b < free_blocks[best].bytes)) best = i;
    }
    if (best < 0) return Entry{0, nullptr};
    const Entry e = free_blocks[best];
    free_blocks.erase(free_blocks.begin() + best);
    return e;
  }
  void give(size_t bytes, double* ptr) { free_blocks.push_back(Entry{bytes, ptr}); }
  size_t bytes() const {
    size_t total = 0;
    for (const Entry& e : free_blocks) total += e.bytes;
    return total;
  }
  // free from the back until at most max_bytes and max_count are kept
  template <class Free>
  void trim(size_t max_bytes, size_t max_count, Free&& free_block) {
    size_t total = bytes();
    while (!free_blocks.empty() && (total > max_bytes || free_blocks.size() > max_count)) {
      total -= free_blocks.back().bytes;
      free_block(free_blocks.back().ptr);
      free_blocks.pop_back();
    }
  }
  template <class Free>
  void clear(Free&& free_block) {
    trim(0, 0, free_block);
  }
};

// One block on loan from a pool.  It goes back to ITS pool with its true capacity when the lease goes out of scope — every
// early return of a submission — unless it has been released to a longer-lived owner (a queued gene) first.
class BlockLease {
 public:
  BlockLease() = default;
  // from the pool, else from alloc(need) (a double*; nullptr = failed: the lease is empty).  A block from alloc is `fresh`:
  // the caller clears it on the stream it fills it on.
  template <class Alloc>
  BlockLease(BlockPool& pool, size_t need, bool bounded, Alloc&& alloc) : pool_(&pool) {
    const BlockPool::Entry e = pool.take(need, bounded);
    if (e.ptr) {
      ptr_ = e.ptr, bytes_ = e.bytes;
    } else if ((ptr_ = alloc(need)) != nullptr) {
      bytes_ = need, fresh_ = true;
    }
  }
  BlockLease(BlockLease&& o) noexcept : pool_(o.pool_), ptr_(o.ptr_), bytes_(o.bytes_), fresh_(o.fresh_) { o.ptr_ = nullptr; }
  BlockLease& operator=(BlockLease&& o) noexcept {
    if (this != &o) {
      give_back();
      pool_ = o.pool_, ptr_ = o.ptr_, bytes_ = o.bytes_, fresh_ = o.fresh_;
      o.ptr_ = nullptr;
    }
    return *this;
  }
  BlockLease(const BlockLease&) = delete;
  BlockLease& operator=(const BlockLease&) = delete;
  ~BlockLease() { give_back(); }

  explicit operator bool() const { return ptr_ != nullptr; }
  double* get() const { return ptr_; }
  size_t bytes() const { return bytes_; }
  bool fresh() const { return fresh_; }
  // the block leaves the lease for good (its capacity in *bytes): nothing goes back to the pool
  double* release(size_t* bytes) {
    double* p = ptr_;
    *bytes = bytes_;
    ptr_ = nullptr;
    return p;
  }

 private:
  void give_back() {
    if (ptr_) pool_->give(bytes_, ptr_);
    ptr_ = nullptr;
  }
  BlockPool* pool_ = nullptr;
  double* ptr_ = nullptr;
  size_t bytes_ = 0;
  bool fresh_ = false;
};

}  // namespace rvt
