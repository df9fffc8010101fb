// Host-only check of eftpipe_amd/csrc/eftb_own.hpp (tests/test_own_host.py compiles and runs it under the address and
// undefined-behaviour sanitizers).  Handles come from malloc, the releaser frees them and writes down which one it was: every expected
// order below is written out by hand, and whatever a ledger failed to release the leak checker reports when the program ends.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eftb_own.hpp"

using namespace eftb;

static int failures = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// a handle is a malloc'ed int that holds its own tag; the releaser logs the tag and frees it
static std::vector<int> released;
static int acquired = 0;

static void* acquire(int tag) {
    int* p = static_cast<int*>(std::malloc(sizeof(int)));
    *p = tag;
    ++acquired;
    return p;
}

static void drop(void* p) {
    released.push_back(*static_cast<int*>(p));
    std::free(p);
}

static void check_log(std::vector<int> want, int line) {
    if (released != want) {
        std::printf("line %d: released", line);
        for (int t : released) std::printf(" %d", t);
        std::printf(", expected");
        for (int t : want) std::printf(" %d", t);
        std::printf("\n");
        ++failures;
    }
    released.clear();
}
#define LOG(...) check_log({__VA_ARGS__}, __LINE__)

int main() {
    int total = 0;  // handles released so far, summed over the logs checked below

    {   // the destructor releases newest first
        Ledger l;
        for (int t : {1, 2, 3, 4}) l.hold(acquire(t), drop);
        LOG();
    }
    LOG(4, 3, 2, 1);
    total += 4;

    {   // release(h): its releaser runs once, now; the destructor does not run it again.  Null and unknown handles are ignored
        Ledger l;
        void* h[3] = {acquire(10), acquire(11), acquire(12)};
        for (void* p : h) l.hold(p, drop);
        l.release(h[1]);
        LOG(11);
        l.release(h[1]);  // (no longer held: compared by address only, never dereferenced)
        l.release(nullptr);
        int other = 0;
        l.release(&other);
        LOG();
        l.release(h[0]);  // the oldest
        LOG(10);
        l.hold(acquire(13), drop);
    }
    LOG(13, 12);
    total += 4;

    {   // release_to(mark): only what came after the mark, newest first; the rest waits for the destructor
        Ledger l;
        l.hold(acquire(20), drop);
        l.hold(acquire(21), drop);
        const Ledger::Mark m = l.mark();
        l.release_to(m);  // nothing since the mark
        LOG();
        for (int t : {22, 23, 24}) l.hold(acquire(t), drop);
        l.release_to(m);
        LOG(24, 23, 22);
        l.release_to(m);
        LOG();
    }
    LOG(21, 20);
    total += 5;

    {   // marked, grown, rolled back, grown again (a set-up that failed and was repeated): every handle released once
        Ledger l;
        l.hold(acquire(30), drop);
        const Ledger::Mark m = l.mark();
        void* grown = acquire(31);
        l.hold(grown, drop);
        l.hold(acquire(32), drop);
        l.release(grown);  // (a buffer that grew inside the set-up: behind the mark, so the mark stands)
        LOG(31);
        l.hold(acquire(33), drop);
        l.release_to(m);
        LOG(33, 32);
        const Ledger::Mark m2 = l.mark();
        CHECK(m2 == m);
        for (int t : {34, 35}) l.hold(acquire(t), drop);
    }
    LOG(35, 34, 30);
    total += 6;

    {   // an empty ledger
        Ledger l;
        l.release_to(l.mark());
        l.release(nullptr);
    }
    LOG();

    CHECK(acquired == 19);
    CHECK(total == acquired);  // nothing is left: every handle went through the releaser exactly once (a second time would be a double free)
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
