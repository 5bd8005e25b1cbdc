// sml_comm.cpp -- sml_comm_*: the RCCL communicator of the hybrid loop's ranks and its
// all-gather (sendrecievegrid's gather of the outvecs, mpires.f90:338-430, over xGMI).
#include "sml_comm.hpp"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <thread>

#include "sml_internal.hpp"

using namespace sml;

namespace {

const char *nccl_msg(ncclResult_t r) { return ncclGetErrorString(r); }

#define SML_NCCL(expr)                                                                                       \
    do {                                                                                                     \
        ncclResult_t r_ = (expr);                                                                            \
        if (r_ != ncclSuccess) return ::sml::fail(SML_ERR_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #expr, nccl_msg(r_)); \
    } while (0)

}  // namespace

extern "C" int sml_comm_unique_id(unsigned char *id) {
    SML_REQUIRE(id, "null argument");
    ncclUniqueId u;
    SML_NCCL(ncclGetUniqueId(&u));
    std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
    return SML_OK;
}

extern "C" int sml_comm_create(int world, int rank, const unsigned char *id, sml_comm **out) {
    SML_REQUIRE(out && world >= 1 && rank >= 0 && rank < world && id, "bad argument");
    *out = nullptr;
    sml_comm *c = new (std::nothrow) sml_comm();
    if (!c) return fail(SML_ERR_NOMEM, "host allocation failed");
    ncclUniqueId u;
    std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    ncclResult_t r = ncclCommInitRank(&c->comm, world, u, rank);
    if (r != ncclSuccess) {
        delete c;
        return fail(SML_ERR_HIP, "ncclCommInitRank(%d of %d): %s", rank, world, nccl_msg(r));
    }
    c->world = world;
    c->rank = rank;
    *out = c;
    return SML_OK;
}

// rank 0 writes the unique id to `path` (atomically: temp file + rename), the other
// ranks wait for it -- the rendezvous a host without MPI needs
extern "C" int sml_comm_create_file(int world, int rank, const char *path, int timeout_s, sml_comm **out) {
    SML_REQUIRE(out && path && world >= 1 && rank >= 0 && rank < world, "bad argument");
    unsigned char id[NCCL_UNIQUE_ID_BYTES];
    if (rank == 0) {
        if (int rc = sml_comm_unique_id(id)) return rc;
        std::string tmp = std::string(path) + ".tmp";
        FILE *f = std::fopen(tmp.c_str(), "wb");
        if (!f) return fail(SML_ERR_IO, "cannot write %s", tmp.c_str());
        const size_t w = std::fwrite(id, 1, sizeof id, f);
        std::fclose(f);
        if (w != sizeof id || std::rename(tmp.c_str(), path) != 0) return fail(SML_ERR_IO, "cannot publish %s", path);
    } else {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            FILE *f = std::fopen(path, "rb");
            if (f) {
                const size_t r = std::fread(id, 1, sizeof id, f);
                std::fclose(f);
                if (r == sizeof id) break;
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(timeout_s > 0 ? timeout_s : 60))
                return fail(SML_ERR_IO, "timed out waiting for %s", path);
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
        }
    }
    return sml_comm_create(world, rank, id, out);
}

// a rank descriptor without a transport: world and rank for sml_hybrid_create when
// the host moves the outvec slabs itself (sml_hybrid_advance_slabs)
extern "C" int sml_comm_create_local(int world, int rank, sml_comm **out) {
    SML_REQUIRE(out && world >= 1 && rank >= 0 && rank < world, "bad argument");
    *out = nullptr;
    sml_comm *c = new (std::nothrow) sml_comm();
    if (!c) return fail(SML_ERR_NOMEM, "host allocation failed");
    c->world = world;
    c->rank = rank;
    *out = c;
    return SML_OK;
}

extern "C" int sml_comm_destroy(sml_comm *c) {
    if (!c) return SML_OK;
    if (c->comm) (void)ncclCommDestroy(c->comm);
    delete c;
    return SML_OK;
}

extern "C" int sml_comm_rank(const sml_comm *c, int *world, int *rank) {
    SML_REQUIRE(c, "null communicator");
    if (world) *world = c->world;
    if (rank) *rank = c->rank;
    return SML_OK;
}

extern "C" int sml_comm_allgather(sml_comm *c, const double *d_send, double *d_recv, int64_t count, void *stream) {
    SML_REQUIRE(c && d_send && d_recv && count >= 0, "bad argument");
    if (!c->comm) return fail(SML_ERR_STATE, "rank %d of %d is a local descriptor without a transport", c->rank, c->world);
    SML_NCCL(ncclAllGather(d_send, d_recv, (size_t)count, ncclDouble, c->comm, (hipStream_t)stream));
    return SML_OK;
}
