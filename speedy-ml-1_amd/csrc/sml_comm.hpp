// sml_comm.hpp -- the communicator of the hybrid loop's ranks: the startup communicator
// (startmpi, mpires.f90:21-37) as an RCCL communicator, or a rank descriptor without a
// transport for a host that moves the outvec slabs itself (sml_comm.cpp).
#pragma once

#include <rccl/rccl.h>

struct sml_comm {
    ncclComm_t comm = nullptr;  // null: a local descriptor (sml_comm_create_local)
    int world = 1, rank = 0;
    bool has_transport() const { return comm != nullptr; }
};
