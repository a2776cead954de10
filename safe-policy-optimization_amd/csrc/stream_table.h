// The table behind every "one block per (device, stream), made at first use, kept until spo_update_scratch_release" of the update
// kernels: a fixed array of CAP blocks keyed by the device ordinal and the raw stream handle (and, where a stream holds more than
// one block, the block's `idx`).  Bookkeeping only: no HIP call and no HIP header -- the caller passes the device ordinal in,
// allocates before add() and frees in release()'s callback -- and no lock: the caller holds the form's mutex around every call.
// Block: a value type with members `int dev; void* stream;` (and `int idx;` where find / add are given one); Block{} is "empty".
#pragma once

namespace spo {

template <class Block, int CAP>
struct StreamTable {
  Block e[CAP] = {};
  int n = 0;

  bool full() const { return n == CAP; }

  // the block of (dev, stream) -- of (dev, stream, idx) -- or null
  Block* find(int dev, const void* stream) {
    return first([&](const Block& b) { return b.dev == dev && b.stream == stream; });
  }
  Block* find(int dev, const void* stream, int idx) {
    return first([&](const Block& b) { return b.dev == dev && b.stream == stream && b.idx == idx; });
  }

  // Appends b (its key is not in the table: the caller has looked) and returns its place, or null when CAP blocks are held: the
  // caller words the refusal or does without a block.  A place is good until the next release().
  Block* add(const Block& b) {
    if (full()) return nullptr;
    e[n] = b;
    return &e[n++];
  }

  // Removes the blocks of (dev, stream_or_null) -- every block of dev when all != 0 --, free_fn(block) once on each before it goes
  // (the last block moves into the gap), and returns how many went.
  template <class Free>
  int release(int dev, const void* stream_or_null, int all, Free free_fn) {
    int freed = 0;
    for (int i = 0; i < n;) {
      if (e[i].dev == dev && (all || e[i].stream == stream_or_null)) {
        free_fn(e[i]);
        e[i] = e[--n];
        e[n] = Block{};
        ++freed;
      } else ++i;
    }
    return freed;
  }

 private:
  template <class Match>
  Block* first(Match match) {
    for (int i = 0; i < n; ++i)
      if (match(e[i])) return &e[i];
    return nullptr;
  }
};

}  // namespace spo
