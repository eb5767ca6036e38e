// device_hold.h -- who owns a decoded result while device-resident batches of it are out (orcgpu_export_device.inc).
//
// The host exports copy a result to pinned memory and count references on that copy (HostMirror::refs); a device export hands
// out the result's own HBM buffers, so the references are on the result itself.  A result has one OWNER -- the caller of the
// decode, or the file reader that decoded it -- and any number of EXPORTS: ArrowDeviceArrays and DLPack tensors.  The owner being
// done with it (orcgpu_result_free, the reader moving on to the next stripe, orcgpu_reader_close) frees or recycles it only when
// no export is out; otherwise it is PARKED and the last export's release decides: back to the reader's spare list (its Home)
// while the reader is open, freed otherwise.  Exactly one of the two ever happens, whichever threads the calls come from.
//
// Pure C++ (no HIP, no types of the library): tests/hostcheck/device_hold_check.cpp runs it under the sanitizers on the CPU.
#pragma once
#include <memory>
#include <mutex>
#include <vector>

namespace orcgpu_hold {

// A reader's spare results: the ones no export holds, which a later stripe is decoded into.  Shared with the holds of the
// reader's results, so that a release after orcgpu_reader_close still finds it -- closed.
struct Home {
  std::mutex m;
  bool open = true;
  std::vector<void*> spare;
};

struct Hold {
  std::mutex m;
  int exports = 0;       // ArrowDeviceArrays and DLPack tensors that view the result
  bool parked = false;   // the owner is done with it: the last release recycles or frees it
  void* payload = nullptr;            // the result
  void (*destroy)(void*) = nullptr;   // frees it (not the Hold)
  std::shared_ptr<Home> home;         // null: a result outside a reader
};

inline Hold* hold_new(void* payload, void (*destroy)(void*), std::shared_ptr<Home> home) {
  Hold* h = new Hold();
  h->payload = payload;
  h->destroy = destroy;
  h->home = std::move(home);
  return h;
}

// h->m is held: the result goes back to its reader's spare list if that reader is still open
inline bool hold_try_recycle(Hold* h) {
  if (!h->home) return false;
  std::lock_guard<std::mutex> g(h->home->m);
  if (!h->home->open) return false;
  h->parked = false;
  h->home->spare.push_back(h->payload);
  return true;
}

inline void hold_acquire(Hold* h) {
  std::lock_guard<std::mutex> g(h->m);
  h->exports++;
}

// Whether an export views the result right now (its owner must not decode into it again)
inline bool hold_exported(Hold* h) {
  std::lock_guard<std::mutex> g(h->m);
  return h->exports > 0;
}

// An export is released.  The last one of a parked result recycles or frees it.
inline void hold_release(Hold* h) {
  {
    std::lock_guard<std::mutex> g(h->m);
    if (--h->exports > 0 || !h->parked) return;
    if (hold_try_recycle(h)) return;
  }
  h->destroy(h->payload);
  delete h;
}

// The owner is done with the result.  recycle: it may go to the spare list (the reader moving on); else it is to be freed
// (orcgpu_result_free, orcgpu_reader_close).  Either happens now when no export is out, and at the last release otherwise.
inline void hold_owner_done(Hold* h, bool recycle) {
  {
    std::lock_guard<std::mutex> g(h->m);
    if (h->exports > 0) {
      h->parked = true;
      return;
    }
    if (recycle && hold_try_recycle(h)) return;
  }
  h->destroy(h->payload);
  delete h;
}

// A spare result to decode into again, or null: a result an export still holds is never in the list.
inline void* home_take(Home& home) {
  std::lock_guard<std::mutex> g(home.m);
  if (home.spare.empty()) return nullptr;
  void* p = home.spare.back();
  home.spare.pop_back();
  return p;
}

// The reader closes: nothing comes home any more; the spare results are the caller's to free.
inline std::vector<void*> home_close(Home& home) {
  std::lock_guard<std::mutex> g(home.m);
  home.open = false;
  std::vector<void*> out;
  out.swap(home.spare);
  return out;
}

}  // namespace orcgpu_hold
