// Test infrastructure (CPU only): csrc/host_batch.hpp, the worker loop the host halves of the input formats share, on its own.
// 64 items on 1, 4 and 16 workers, items 9, 40 and 41 fail: the failure returned is always item 9's, status and text, no item
// runs twice, every item below 9 runs, and with one worker nothing past 9 runs; a batch where nothing fails runs every item
// once, and an empty batch runs nothing.  Repeated, so that the sanitizers (AddressSanitizer + UBSan, or ThreadSanitizer)
// meet more than one interleaving.  tests/test_decode_stage_cpu.py builds and runs it:
//   g++ -fsanitize=... host_batch_check.cpp        prints "host_batch ok"
#include <stdio.h>
#include <string.h>

#include <atomic>

#include "../../vip-cup-2022_amd/csrc/host_batch.hpp"

using Err = host_batch::Err<-42>;

static int check(bool ok, const char* what, int threads) {
    if (!ok) fprintf(stderr, "host_batch_check: %s (threads = %d)\n", what, threads);
    return ok ? 0 : 1;
}

int main() {
    const int N = 64;
    int wrong = 0;
    const int workers[3] = {1, 4, 16};
    for (int threads : workers) {
        for (int round = 0; round < 200; ++round) {
            std::atomic<int> runs[N];
            for (auto& r : runs) r.store(0);
            const auto failed = host_batch::run<Err>(N, threads, [&](int i, Err& e) {
                runs[i].fetch_add(1);
                if (i == 9 || i == 40 || i == 41) return fail(e, "item %d is bad", i) - i;      // a status of its own per item
                return 0;
            });
            wrong += check(failed.status == -42 - 9 && failed.index == 9, "the failure returned is not item 9's", threads);
            wrong += check(strcmp(failed.err.msg, "item 9 is bad") == 0, "the text returned is not item 9's", threads);
            for (int i = 0; i < N; ++i) {
                wrong += check(runs[i].load() <= 1, "an item ran twice", threads);
                if (i <= 9) wrong += check(runs[i].load() == 1, "an item up to the failing one did not run", threads);
                if (i > 9 && threads == 1) wrong += check(runs[i].load() == 0, "one worker went on after the failure", threads);
            }
            for (auto& r : runs) r.store(0);
            const auto fine = host_batch::run<Err>(N, threads, [&](int i, Err&) { return runs[i].fetch_add(1) * 0; });
            wrong += check(fine.status == 0 && fine.index == -1 && fine.err.msg[0] == 0, "a failure out of a batch without one", threads);
            for (int i = 0; i < N; ++i) wrong += check(runs[i].load() == 1, "an item of a good batch did not run exactly once", threads);
            const auto none = host_batch::run<Err>(0, threads, [](int, Err&) { return 1; });
            wrong += check(none.status == 0, "an empty batch failed", threads);
            if (wrong) return 1;
        }
    }
    printf("host_batch ok\n");
    return 0;
}
