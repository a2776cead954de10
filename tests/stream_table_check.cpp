// Stand-alone check of csrc/stream_table.h (built and run by tests/test_stream_table_host.py with the host compiler: the header makes
// no HIP call and includes no HIP header).  Prints one "ok <property>" line per property that holds, "FAIL <property>: <why>"
// otherwise, and "done <failures>" last; exits 1 when anything failed.
#include <cstdio>
#include <cstdint>
#include <set>
#include <vector>
#include "stream_table.h"

namespace {

struct Block { int dev; void* stream; int idx; int id; };
constexpr int CAP = 6;
using Table = spo::StreamTable<Block, CAP>;

int g_failures = 0;
void report(const char* what, bool ok, const char* why = "") {
  if (ok) printf("ok %s\n", what);
  else { printf("FAIL %s: %s\n", what, why); ++g_failures; }
}

void* stream(int k) { return reinterpret_cast<void*>(static_cast<uintptr_t>(0x1000 + 0x40 * k)); }

}  // namespace

int main() {
  // ---- find after add; distinct (device, stream, idx) keys give distinct blocks
  {
    Table t;
    bool ok = t.find(0, stream(1)) == nullptr && t.find(0, stream(1), 0) == nullptr;
    Block* a = t.add(Block{0, stream(1), 0, 10});
    Block* b = t.add(Block{0, stream(1), 1, 11});                 // same stream, second block
    Block* c = t.add(Block{0, stream(2), 0, 12});                 // other stream
    Block* d = t.add(Block{1, stream(1), 0, 13});                 // same handle on another device
    ok = ok && a && b && c && d;
    report("find after add", ok && t.find(0, stream(1), 0) == a && t.find(0, stream(1), 1) == b && t.find(0, stream(2)) == c &&
                                 t.find(1, stream(1)) == d && t.find(1, stream(1), 0) == d && a->id == 10 && d->id == 13);
    std::set<Block*> places{a, b, c, d};
    report("distinct keys give distinct blocks", places.size() == 4 && t.n == 4 && t.find(0, stream(2), 1) == nullptr &&
                                                     t.find(1, stream(2)) == nullptr && t.find(2, stream(1)) == nullptr);
  }
  // ---- add fails at CAP and not before
  {
    Table t;
    bool ok = true;
    for (int k = 0; k < CAP; ++k) {
      ok = ok && !t.full();
      ok = ok && t.add(Block{0, stream(k), 0, k}) != nullptr;
    }
    report("add succeeds CAP times", ok && t.n == CAP);
    report("add fails at CAP", t.full() && t.add(Block{0, stream(CAP), 0, CAP}) == nullptr && t.n == CAP &&
                                   t.find(0, stream(CAP)) == nullptr);
    bool kept = true;
    for (int k = 0; k < CAP; ++k) kept = kept && t.find(0, stream(k)) && t.find(0, stream(k))->id == k;
    report("a refused add leaves the table as it was", kept);
  }
  // ---- release by stream / with all; the callback; swap-remove; adding a released key again
  {
    Table t;
    // device 0: stream 1 (idx 0 and 1), stream 2, stream 3; device 1: stream 1, stream 2  -- stream 1's blocks first, so that
    // the swap-remove moves later blocks into their places
    t.add(Block{0, stream(1), 0, 100});
    t.add(Block{0, stream(1), 1, 101});
    t.add(Block{0, stream(2), 0, 102});
    t.add(Block{1, stream(1), 0, 103});
    t.add(Block{0, stream(3), 0, 104});
    t.add(Block{1, stream(2), 0, 105});
    std::vector<int> freed;
    auto free_fn = [&](Block& b) { freed.push_back(b.id); };
    int n = t.release(0, stream(1), 0, free_fn);
    report("release by stream returns the stream's block count", n == 2 && t.n == 4);
    report("release by stream removes exactly that stream's blocks on that device",
           !t.find(0, stream(1), 0) && !t.find(0, stream(1), 1) && !t.find(0, stream(1)) && t.find(1, stream(1)) && t.find(0, stream(2)) &&
               t.find(0, stream(3)) && t.find(1, stream(2)));
    report("the callback runs once per removed block", freed.size() == 2 && std::set<int>(freed.begin(), freed.end()) == std::set<int>{100, 101});
    report("swap-remove leaves the survivors findable", t.find(0, stream(2))->id == 102 && t.find(1, stream(1))->id == 103 &&
                                                            t.find(0, stream(3))->id == 104 && t.find(1, stream(2))->id == 105);
    freed.clear();
    report("releasing a stream without blocks returns 0", t.release(0, stream(1), 0, free_fn) == 0 && freed.empty() && t.n == 4);
    report("a null stream without all releases nothing", t.release(0, nullptr, 0, free_fn) == 0 && freed.empty() && t.n == 4);
    Block* again = t.add(Block{0, stream(1), 0, 200});
    report("a released key can be added again", again && t.find(0, stream(1), 0) == again && again->id == 200 && t.n == 5);
    n = t.release(0, nullptr, 1, free_fn);
    report("release with all empties that device only", n == 3 && t.n == 2 && !t.find(0, stream(1)) && !t.find(0, stream(2)) &&
                                                            !t.find(0, stream(3)) && t.find(1, stream(1)) && t.find(1, stream(1))->id == 103 &&
                                                            t.find(1, stream(2)) && t.find(1, stream(2))->id == 105);
    report("the callback runs once per block of the device", freed.size() == 3 &&
                                                                 std::set<int>(freed.begin(), freed.end()) == std::set<int>{102, 104, 200});
    freed.clear();
    n = t.release(1, stream(7), 1, free_fn);                       // all != 0: the stream argument does not matter
    report("release with all ignores the stream argument", n == 2 && t.n == 0 && freed.size() == 2);
    bool room = true;
    for (int k = 0; k < CAP; ++k) room = room && t.add(Block{0, stream(k), 0, k}) != nullptr;
    report("an emptied table takes CAP blocks again", room && t.full());
  }
  printf("done %d\n", g_failures);
  return g_failures ? 1 : 0;
}
