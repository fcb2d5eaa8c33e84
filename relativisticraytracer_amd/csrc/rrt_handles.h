/*
 * rrt_handles.h -- the one registry behind the library's five kinds of handle (sky, workspace, noise table, tile map, tile order).
 * A handle is an id into a process-wide table, never a raw pointer: a stale or made-up id is reported (RRT_ERR_BAD_HANDLE) instead
 * of being dereferenced.  Plain C++: no HIP type, no device code, so that a host-only test can compile it
 * (tests/handles/handle_exerciser.cpp).  The five instances and the helper that adds the device check (lookup_here) are in
 * rrt_hip.hip; the object structs are there, in rrt_noise_plan.h and in rrt_tile_objects.h.
 *
 * The table owns the mutex, the map and the id counter, and every operation is ONE critical section that copies the element out:
 * nothing of a caller ever runs under the lock except take()'s predicate, and no reference into the map leaves it.  The element
 * is the object itself (sky, workspace, noise table: small structs of device pointers, copied per launch) or a shared_ptr to it
 * (tile map, tile order: objects with vectors or a mutex of their own, pinned by the copy while a launch uses them).  Ids count
 * up from the instance's first id and are never issued twice, so an id that was destroyed stays unknown for good.
 * There is no with(id, f) that runs f under the lock: rrt_noise_table_info and _window, which used to read in place, copy the
 * NoiseTableObject out with get() like every launch already does (about 6 KB: BandPlan's 64-band arrays) -- a query is no hot path.
 *
 * WHAT THE ENTRY POINTS DO DIFFERENTLY ON PURPOSE.  These differences are contract (tests pin the return codes); the table
 * serves all of them and harmonises none:
 *   - Destroy checks the device only for tile map and tile order: inside the lock, before the erase (take()'s predicate), so a
 *     destroy under another device is RRT_ERR_BAD_HANDLE and the object stays registered.  Sky, workspace and noise table are
 *     destroyed from any device (take() without a predicate).
 *   - rrt_noise_table_info and _window do not check the device.  rrt_workspace_read checks its arguments before the device;
 *     rrt_workspace_stats and _rounds check the device before the copy.  rrt_tile_map_shard_rows, rrt_tile_order_set_seeding and
 *     _seeded do not check it; rrt_tile_order_info checks it after taking the object's mutex.
 *   - Tile order keeps its own per-object mutex and its `dead` flag: the table's lock covers only the lookup, so threads driving
 *     different objects never wait for each other.  rrt_tile_order_destroy takes the object's mutex AFTER the erase,
 *     and a launch that was waiting for that mutex finds `dead` set.
 *   - fill_args rejects a stale or foreign rrt_params.tile_order whatever path the launch takes, and looks the sky up first, the
 *     tile order second, the noise table third; launch() takes the tile order (its mutex) only after all of that.
 *   - rrt_noise_table_create_window records hipGetDevice(), not current_device(): a fake device does not reach it.
 *   - rrt_sky_create_from_device asks hipPointerGetAttributes for the owning device unless a fake device is set.
 *   - The texts left in rrt_last_hip_error() are those of the HIP calls around the table; the table itself writes none.
 */
#ifndef RRT_HANDLES_H
#define RRT_HANDLES_H

#include <cstddef>
#include <mutex>
#include <unordered_map>
#include <utility>

namespace rrt_handles {

enum Taken {
    kTaken = 0,      /* erased and copied out */
    kUnknown = 1,    /* no such id; the table is as it was */
    kRefused = 2     /* the predicate said no; the element stays registered */
};

template <class Id, class T>
class HandleTable {
  public:
    explicit HandleTable(Id first) : next_(first) {}
    HandleTable(const HandleTable&) = delete;
    HandleTable& operator=(const HandleTable&) = delete;

    Id insert(T v) {
        std::lock_guard<std::mutex> lk(mu_);
        const Id id = next_++;
        map_.emplace(id, std::move(v));
        return id;
    }
    /* a copy of the element (a shared_ptr element: a second owner) */
    bool get(Id id, T& out) {
        std::lock_guard<std::mutex> lk(mu_);
        const auto it = map_.find(id);
        if (it == map_.end()) return false;
        out = it->second;
        return true;
    }
    /* find, ask accept(element), erase, copy out: one critical section */
    template <class Pred>
    Taken take(Id id, T& out, Pred accept) {
        std::lock_guard<std::mutex> lk(mu_);
        const auto it = map_.find(id);
        if (it == map_.end()) return kUnknown;
        if (!accept(static_cast<const T&>(it->second))) return kRefused;
        out = std::move(it->second);
        map_.erase(it);
        return kTaken;
    }
    Taken take(Id id, T& out) {
        return take(id, out, [](const T&) { return true; });
    }
    size_t size() {
        std::lock_guard<std::mutex> lk(mu_);
        return map_.size();
    }

  private:
    std::mutex mu_;
    std::unordered_map<Id, T> map_;
    Id next_;
};

}  // namespace rrt_handles

#endif
