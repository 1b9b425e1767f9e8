// What the host halves of the input formats (jpeg / png / webp / vp8 _host.cpp) share: the error text of one image, and the
// loop that decodes the images of a batch on a few worker threads.  Plain C++, no HIP, no other header of the project: the
// fuzz harnesses compile one *_host.cpp alone and find this file next to it.
#pragma once

#include <stdarg.h>
#include <stdio.h>

#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

namespace host_batch {

// Error text of one image, formatted where the failure is found (a worker thread) and reported by the thread that made the
// call: vip_set_error's buffer is thread_local, so a worker must not use it.  STATUS: the vip_status its format fails with.
template <int STATUS>
struct Err {
    char msg[256] = "";
};

template <int STATUS>
int fail(Err<STATUS>& e, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(e.msg, sizeof(e.msg), fmt, ap);
    va_end(ap);
    return STATUS;
}

// Of the items that failed, the one with the lowest index: its status, index and text.  status 0: none failed.
template <class E>
struct Failure {
    int status = 0, index = -1;
    E err;
};

// Run ``int work(int i, E& e)`` (0 = ok) for i = 0 .. n-1, one item at a time per worker; threads <= 1 runs inline, in order.
// Items are handed out in index order and an item is skipped only when a lower one has already failed, so which failure is
// returned does not depend on the timing: it is the one a single worker would have stopped at.
template <class E, class Work>
Failure<E> run(int n, int threads, Work work) {
    Failure<E> first;
    std::atomic<int> next(0), bad(n);
    std::mutex mu;
    auto loop = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n || i > bad.load()) return;
            E e;
            const int st = work(i, e);
            if (st != 0) {
                std::lock_guard<std::mutex> g(mu);
                if (i < bad.load()) {
                    bad.store(i);
                    first.status = st;
                    first.index = i;
                    first.err = e;
                }
            }
        }
    };
    if (threads <= 1) {
        loop();
    } else {
        std::vector<std::thread> pool;
        for (int t = 0; t < threads; ++t) pool.emplace_back(loop);
        for (auto& t : pool) t.join();
    }
    return first;
}

}  // namespace host_batch
