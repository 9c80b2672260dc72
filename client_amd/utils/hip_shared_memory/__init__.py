"""HIP-IPC shared-memory utilities — the MI355X data plane.

API-compatible with ``tritonclient.utils.cuda_shared_memory`` (reference:
tritonclient/utils/cuda_shared_memory/__init__.py — every public
function keeps its name and signature) but implemented on HIP:
hipMalloc + hipIpcGetMemHandle on the client, the server opens with
hipIpcOpenMemHandle, and tensors stay resident in the MI355X's 288 GB
HBM3E instead of crossing PCIe.

Beyond the reference API this module adds device-side pack/unpack:
``set_shared_memory_region_cast`` uploads fp32 once and runs the CDNA4
cast kernel (fp32->bf16 wire-exact truncation, or fp32->fp8 e4m3) into
the region — replacing the reference's per-element CPU BF16 loop
(reference utils/__init__.py:294-363, SURVEY.md §2.9 rows ★2/★11).
"""

import base64

import numpy as np

from .. import serialize_byte_tensor
from .._dlpack import (
    DLDeviceType,
    get_byte_size,
    get_dlpack_capsule,
    get_managed_tensor,
    is_contiguous_data,
)
from .._shared_memory_tensor import SharedMemoryTensor
from ...ops import hip_runtime as hr

allocated_shm_regions = []


class CudaSharedMemoryException(Exception):
    def __init__(self, err):
        self.err_ = err
        super().__init__(str(err))

    def __str__(self):
        return self.err_ if isinstance(self.err_, str) else str(self.err_)


# AMD-native alias
HipSharedMemoryException = CudaSharedMemoryException


class CudaSharedMemoryRegion:
    """Tracks one hipMalloc'd region and frees it on destruction
    (reference _utils.py:88-100)."""

    def __init__(self, triton_shm_name, byte_size, device_id):
        self._triton_shm_name = triton_shm_name
        self._byte_size = byte_size
        self._device_id = device_id
        self._base_addr = hr.malloc(device_id, byte_size)
        self._scratch = 0
        self._scratch_size = 0
        self._closed = False

    def ptr(self):
        return self._base_addr

    def _ensure_scratch(self, nbytes):
        if self._scratch_size < nbytes:
            if self._scratch:
                hr.free(self._scratch)
            self._scratch = hr.malloc(self._device_id, nbytes)
            self._scratch_size = nbytes
        return self._scratch

    def close(self):
        if not self._closed:
            self._closed = True
            if self._scratch:
                hr.free(self._scratch)
                self._scratch = 0
            hr.free(self._base_addr)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


HipSharedMemoryRegion = CudaSharedMemoryRegion


def create_shared_memory_region(triton_shm_name, byte_size, device_id):
    """hipSetDevice -> hipMalloc -> track (reference :107-149)."""
    try:
        handle = CudaSharedMemoryRegion(triton_shm_name, byte_size, device_id)
    except RuntimeError as e:
        raise CudaSharedMemoryException(
            f"unable to create HIP shared memory region: {e}"
        )
    allocated_shm_regions.append(handle)
    return handle


def get_raw_handle(shm_handle):
    """base64-encoded 64-byte hipIpcMemHandle_t (reference :152-170)."""
    raw = hr.ipc_get_mem_handle(shm_handle._base_addr)
    return base64.b64encode(raw)


def get_raw_handle_bytes(shm_handle):
    """The raw (un-encoded) handle bytes, for the gRPC register call."""
    return hr.ipc_get_mem_handle(shm_handle._base_addr)


def set_shared_memory_region(shm_handle, input_values, offset=0):
    """Copy numpy tensors into the device region via hipMemcpyAsync on the
    region's cached stream (reference :173-239)."""
    if not isinstance(input_values, (list, tuple)):
        raise CudaSharedMemoryException(
            "input_values must be specified as a list/tuple of numpy arrays"
        )
    cur = offset
    for input_value in input_values:
        input_value = np.ascontiguousarray(input_value)
        if input_value.dtype == np.object_:
            byte_data = serialize_byte_tensor(input_value).item()
            arr = np.frombuffer(byte_data, dtype=np.uint8)
        else:
            arr = input_value.reshape(-1).view(np.uint8)
        nbytes = arr.nbytes
        if cur + nbytes > shm_handle._byte_size:
            raise CudaSharedMemoryException(
                "input exceeds shared memory region size"
            )
        hr.memcpy_h2d(shm_handle._base_addr + cur, arr, nbytes,
                      shm_handle._device_id, True)
        cur += nbytes


_CAST_WIRE_ITEMSIZE = {"BF16": 2, "FP8E4M3": 1, "FP32": 4}


def _check_cast_range(shm_handle, wire_datatype, n, offset):
    """The cast kernels write/read n wire elements at base + offset; the
    whole range must lie inside the region (nothing is launched
    otherwise)."""
    itemsize = _CAST_WIRE_ITEMSIZE.get(wire_datatype)
    if itemsize is None:
        raise CudaSharedMemoryException(
            f"unsupported cast datatype {wire_datatype}"
        )
    if offset < 0:
        raise CudaSharedMemoryException("offset must be non-negative")
    if offset + n * itemsize > shm_handle._byte_size:
        raise CudaSharedMemoryException(
            "cast range exceeds shared memory region size"
        )


def set_shared_memory_region_cast(shm_handle, input_value, wire_datatype,
                                  offset=0, sync=True):
    """MI355X pack path: upload fp32 host data to device scratch once,
    then run the CDNA4 cast kernel into the region (bf16 wire-exact
    truncation / fp8 e4m3 RNE). Returns the packed byte size.

    FP8E4M3 contract (OCP e4m3fn codes): round to nearest, ties to the
    even code (subnormal step 2**-9); finite values that round above 448
    saturate to +-448 (codes 0x7E / 0xFE) — unlike
    ``torch.float8_e4m3fn``, which turns everything above 464 into NaN;
    NaN and +-Inf give a NaN code (``code & 0x7F == 0x7F``); the sign of
    a zero result is preserved.

    Raises CudaSharedMemoryException, before anything is uploaded or
    launched, if ``[offset, offset + packed size)`` does not lie inside
    the region."""
    arr = np.ascontiguousarray(input_value, dtype=np.float32)
    n = arr.size
    _check_cast_range(shm_handle, wire_datatype, n, offset)
    scratch = shm_handle._ensure_scratch(arr.nbytes)
    hr.memcpy_h2d(scratch, arr.reshape(-1).view(np.uint8), arr.nbytes,
                  shm_handle._device_id, False)
    dst = shm_handle._base_addr + offset
    if wire_datatype == "BF16":
        hr.cast_fp32_bf16(scratch, dst, n, shm_handle._device_id, sync, 0)
        return n * 2
    elif wire_datatype == "FP8E4M3":
        hr.cast_fp32_fp8e4m3(scratch, dst, n, shm_handle._device_id, sync, 0)
        return n
    elif wire_datatype == "FP32":
        hr.memcpy_d2d(dst, scratch, arr.nbytes, shm_handle._device_id, sync)
        return arr.nbytes
    raise CudaSharedMemoryException(
        f"unsupported cast target datatype {wire_datatype}"
    )


def get_contents_cast(shm_handle, wire_datatype, shape, offset=0):
    """Inverse of set_shared_memory_region_cast: device unpack kernel
    (bf16/fp8 -> fp32) then one D2H copy; returns fp32 numpy. Raises
    CudaSharedMemoryException if the source range leaves the region."""
    n = int(np.prod(shape))
    _check_cast_range(shm_handle, wire_datatype, n, offset)
    scratch = shm_handle._ensure_scratch(n * 4)
    src = shm_handle._base_addr + offset
    if wire_datatype == "BF16":
        hr.cast_bf16_fp32(src, scratch, n, shm_handle._device_id, True, 0)
    elif wire_datatype == "FP8E4M3":
        hr.cast_fp8e4m3_fp32(src, scratch, n, shm_handle._device_id, True, 0)
    elif wire_datatype == "FP32":
        scratch = src
    else:
        raise CudaSharedMemoryException(
            f"unsupported cast source datatype {wire_datatype}"
        )
    out = np.empty(n, dtype=np.float32)
    hr.memcpy_d2h_into(scratch, out.view(np.uint8), n * 4,
                       shm_handle._device_id)
    return out.reshape(shape)


def set_shared_memory_region_from_dlpack(shm_handle, input_values, offset=0):
    """Ingest DLPack tensors (device or host). Contiguous tensors are one
    hipMemcpyAsync; strided device tensors go through the gather_pack
    kernel — the reference rejects non-contiguous input
    (reference :328-388)."""
    if not isinstance(input_values, (list, tuple)):
        raise CudaSharedMemoryException(
            "input_values must be specified as a list/tuple of DLPack tensors"
        )
    cur = offset
    for value in input_values:
        capsule = get_dlpack_capsule(value)
        managed = get_managed_tensor(capsule)
        dt = managed.dl_tensor
        ndim = dt.ndim
        shape = [dt.shape[i] for i in range(ndim)]
        strides = (
            [dt.strides[i] for i in range(ndim)] if dt.strides else None
        )
        byte_size = get_byte_size(dt.dtype, shape)
        src = (dt.data or 0) + dt.byte_offset
        dev_type = dt.device.device_type
        on_device = dev_type in (DLDeviceType.kDLROCM, DLDeviceType.kDLCUDA)
        contiguous = is_contiguous_data(
            ndim, dt.shape, dt.strides if dt.strides else None
        )
        if cur + byte_size > shm_handle._byte_size:
            raise CudaSharedMemoryException(
                "input exceeds shared memory region size"
            )
        dst = shm_handle._base_addr + cur
        if on_device:
            if contiguous:
                hr.memcpy_d2d(dst, src, byte_size, shm_handle._device_id, True)
            else:
                elem = dt.dtype.bits // 8
                hr.gather_pack(src, dst, elem, shape, strides,
                               shm_handle._device_id, True)
        else:
            if not contiguous:
                raise CudaSharedMemoryException(
                    "host DLPack input must be contiguous"
                )
            buf = (np.ctypeslib.as_array(
                __import__("ctypes").cast(
                    src, __import__("ctypes").POINTER(__import__("ctypes").c_uint8)
                ),
                shape=(byte_size,),
            ))
            hr.memcpy_h2d(dst, buf, byte_size, shm_handle._device_id, True)
        cur += byte_size


def get_contents_as_numpy(shm_handle, datatype, shape, offset=0):
    """D2H download + numpy view (reference :242-325). BYTES walks the
    serialized buffer; BF16 is widened to fp32 on device first."""
    from .. import deserialize_bytes_tensor

    if datatype == np.object_ or datatype == bytes:
        raw = hr.memcpy_d2h(
            shm_handle._base_addr + offset,
            shm_handle._byte_size - offset,
            shm_handle._device_id,
        )
        result = deserialize_bytes_tensor(raw)[: int(np.prod(shape))]
        return result.reshape(shape)
    if isinstance(datatype, str) and datatype == "BF16":
        return get_contents_cast(shm_handle, "BF16", shape, offset)
    dt = np.dtype(datatype)
    count = int(np.prod(shape)) if shape else 1
    nbytes = count * dt.itemsize
    out = np.empty(count, dtype=dt)
    hr.memcpy_d2h_into(shm_handle._base_addr + offset, out.view(np.uint8),
                       nbytes, shm_handle._device_id)
    return out.reshape(shape)


def as_shared_memory_tensor(shm_handle, datatype, shape, offset=0):
    """Zero-copy DLPack view (kDLROCM) of the region (reference :391-399)."""
    return SharedMemoryTensor(
        datatype=datatype,
        shape=shape,
        base_addr=shm_handle._base_addr + offset,
        byte_offset=0,
        device_type=DLDeviceType.kDLROCM,
        device_id=shm_handle._device_id,
    )


def allocated_shared_memory_regions():
    return [
        (r._triton_shm_name, r._byte_size, r._device_id)
        for r in allocated_shm_regions
        if not r._closed
    ]


def destroy_shared_memory_region(shm_handle):
    """hipFree the region (reference _utils.py:88-100)."""
    shm_handle.close()
    try:
        allocated_shm_regions.remove(shm_handle)
    except ValueError:
        pass
