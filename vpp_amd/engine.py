"""Host layer of the GPU verdict backend (Python stand-in for the Go host).

``Engine`` wraps the C ABI (include/contivcls.h): compiled rule tables,
batched classification of packet batches resident in HBM (torch tensors) or
host memory (numpy), the device traffic generator.

``ACLEngine`` is the drop-in for the reference's MockACLEngine
(mock/aclengine/aclengine_mock.go:94-471) with the same method set:
RegisterPod, ApplyTxn, DumpACLs, GetNumOfACLs, GetInboundACL,
GetOutboundACL, GetACLByName, GetNumOfACLChanges and the three Connection*
entry points -- plus ``connection_batch`` which evaluates many connections in
one GPU launch.  ACL configuration (interfaces, replace-on-put, change
counting) lives in the C++ engine; this layer keeps only what the Go host
would: the protobuf ACLs by name, pods and interface names.
"""
from __future__ import annotations

import collections
import ctypes as C
import weakref
from typing import Optional

import numpy as np

from . import _abi, gonet
from ._abi import ClsError

ACL_KEY_PREFIX = "vpp/config/v1/acl/"
# ConnectionAction (aclengine_mock.go:46-60)
CONN_DENY_SYN, CONN_DENY_SYN_ACK, CONN_ALLOW, CONN_FAILURE = 0, 1, 2, 3
# ProtocolType (aclengine_mock.go:80-91)
TCP, UDP, ICMP = 0, 1, 2


# Engine.reach_diff's result; what was not asked for is None
ReachDiff = collections.namedtuple("ReachDiff", "verdicts changes n_changes trans changed hist allow")
# Engine.reach_ports's result
ReachPorts = collections.namedtuple("ReachPorts", "ranges n_ranges runs allow_ports hist n_classes")
# Engine.reach_hops's result; what was not asked for is None
ReachHops = collections.namedtuple("ReachHops", "hops reach exposed levels closure")
# Engine.reach_classes's result; verdict is None unless asked for
ReachClasses = collections.namedtuple("ReachClasses", "classes reps sizes self_ quotient rounds verdict")


def expand_classes(classes, self_, quotient) -> np.ndarray:
    """The [P, N, N] matrix that Engine.reach_classes summarised: cell (p, s,
    d) is quotient[p, classes[s], classes[d]] off the diagonal and self_[p,
    classes[s]] on it."""
    c = np.asarray(classes).astype(np.int64)
    q, d = np.asarray(quotient, np.uint8), np.asarray(self_, np.uint8)
    m = np.ascontiguousarray(q[:, c[:, None], c[None, :]])
    at = np.arange(len(c))
    m[:, at, at] = d[:, c]
    return m


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _ptr(x):
    if x is None:
        return None
    if _is_torch(x):
        return x.data_ptr()
    return x.ctypes.data


class Table:
    def __init__(self, engine: "Engine", tid: int, n_rules: int, name: str):
        self.engine = engine
        self.id = tid
        self.n_rules = n_rules
        self.name = name

    def info(self) -> dict:
        inf = _abi.TableInfo()
        self.engine._check(_abi.lib().cls_table_get_info(self.engine.h, self.id, C.byref(inf)))
        return {k: getattr(inf, k) for k, _ in _abi.TableInfo._fields_ if k != "reserved"}


class Engine:
    """One gfx950 device, or (``devices``) a multi-device engine: tables
    compiled once and replicated, batches sharded over the devices, hit
    counters merged by the library's RCCL all-reduce (include/contivcls.h)."""

    def __init__(self, device: int = -1, devices=None, options: Optional[dict] = None):
        L = _abi.lib()
        if devices:
            self._devs = (C.c_int * len(devices))(*devices)
            cfg = _abi.Config(-1, len(devices), C.cast(self._devs, C.POINTER(C.c_int)))
        else:
            cfg = _abi.Config(device, 0, None)
        h = C.c_void_p()
        rc = L.cls_engine_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise ClsError("cls_engine_create failed (rc=%d): %s" % (
                rc, "RCCL communicator" if rc == _abi.E_RCCL else "no usable gfx950 device"))
        self.h = h
        self._owned = True
        self._batches = weakref.WeakSet()       # closed before the engine (cls_engine_destroy)
        self._views = []                        # device_engine() views: invalid once the engine closes
        for k, v in (options or {}).items():
            self.set_option(k, v)

    @classmethod
    def _view(cls, handle) -> "Engine":
        v = cls.__new__(cls)
        v.h = handle
        v._owned = False
        v._batches = weakref.WeakSet()
        v._views = []
        return v

    def set_option(self, key: str, value=None):
        """cls_engine_set_option: a tuning / diagnostic switch of this engine
        (tests and measurements: forced list modes, counter tiers, launch
        plans; include/contivcls.h), ``None`` for its default.  The library
        never reads the environment."""
        v = None if value is None else str(value).encode()
        self._check(_abi.lib().cls_engine_set_option(self.h, key.encode(), v))

    def close(self):
        if getattr(self, "h", None) and getattr(self, "_owned", True):
            # the batches (and borrowed device views) hold this engine's handle
            for b in list(getattr(self, "_batches", ())):
                b.close()
            for v in getattr(self, "_views", ()):
                v.h = None
            _abi.lib().cls_engine_destroy(self.h)
        self.h = None

    # -- devices, batches, the counter all-reduce (ABI 4) -------------------
    def n_devices(self) -> int:
        n = C.c_uint32(0)
        self._check(_abi.lib().cls_engine_devices(self.h, C.byref(n)))
        return n.value

    def device_engine(self, index: int) -> "Engine":
        """Borrowed single-device view of device ``index`` (timing, stream
        floors, raw device pointers of that device)."""
        d = C.c_void_p()
        self._check(_abi.lib().cls_device_engine(self.h, index, C.byref(d)))
        v = Engine._view(d)
        self._views.append(v)
        return v

    def batch(self, n: int, af: int = _abi.AF_V4, conn: bool = False, mirror: bool = False) -> "Batch":
        return Batch(self, n, af, conn, mirror)

    def classify_batch(self, table: Table, batch: "Batch", counters: bool = True, timing: bool = False,
                       no_verdict: bool = False, force_linear: bool = False):
        """cls_classify_batch: verdicts stay in the batch (CLS_BF_VERDICT);
        returns the merged hit counters (uint64[R+1]) or, counters=False,
        None after only enqueueing the work."""
        flags = (_abi.F_TIMING if timing else 0) | (_abi.F_NO_VERDICT if no_verdict else 0) | \
            (_abi.F_FORCE_LINEAR if force_linear else 0)
        out = np.zeros(table.n_rules + 1, np.uint64) if counters else None
        self._check(_abi.lib().cls_classify_batch(self.h, table.id, batch.h, _ptr(out), flags))
        return out

    def connect_batch_b(self, batch: "Batch", mode: str = "auto", count: bool = False):
        """cls_batch_connect: ConnectionAction per connection into the batch."""
        flags = {"auto": 0, "classifier": _abi.F_CONN_CLS, "linear": _abi.F_FORCE_LINEAR}[mode]
        if count:
            flags |= _abi.F_COUNT
        self._check(_abi.lib().cls_batch_connect(self.h, batch.h, flags))

    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = _abi.lib().cls_comm_unique_id(buf)
        if rc != 0:
            raise ClsError("cls_comm_unique_id failed (rc=%d)" % rc)
        return bytes(buf)

    def comm_init(self, n_procs: int = 1, proc: int = 0, uid: Optional[bytes] = None):
        ib = (C.c_uint8 * 128).from_buffer_copy(uid) if uid is not None else None
        self._check(_abi.lib().cls_comm_init(self.h, n_procs, proc, ib))

    def comm_info(self):
        n, r = C.c_uint32(0), C.c_uint32(0)
        self._check(_abi.lib().cls_comm_info(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != 0:
            raise ClsError("rc=%d: %s" % (rc, _abi.lib().cls_last_error(self.h).decode()))

    # -- tables -----------------------------------------------------------
    def put_table(self, name: str, rules) -> Table:
        cr = rules if isinstance(rules, _abi.CRules) else _abi.CRules(rules)
        tid = C.c_uint32(0)
        self._check(_abi.lib().cls_table_put(self.h, name.encode(), cr.ptr(), cr.n, C.byref(tid)))
        return Table(self, tid.value, cr.n, name)

    def del_table(self, table: Table):
        self._check(_abi.lib().cls_table_del(self.h, table.id))

    # -- classify ---------------------------------------------------------
    def classify(self, table: Table, src, dst, dport, proto, verdict=None, counters=None,
                 force_linear=False, timing=False, accumulate=False, stream=None):
        """A packet batch: IPv4 (src, dst: uint32[n], host order) or the
        16-byte layout (src, dst: uint8[n, 16], network order; IPv4-mapped
        addresses are IPv4 packets).  numpy inputs: synchronous, returns
        (verdict, counters) as numpy arrays.  torch device tensors: enqueued on
        ``stream`` (a torch.cuda.Stream or raw handle; default torch's current
        stream); ``verdict`` (uint8[n]) and ``counters`` (int64[R+1]) are
        written."""
        n = int(len(dport))
        dev = _is_torch(src)
        v16 = (src.dim() if dev else np.ndim(src)) == 2

        def soa(s_, d_, dp_, pr_):
            if v16:
                return _abi.PktSoa(_abi.AF_V16, None, None, _ptr(s_), _ptr(d_), None, _ptr(dp_), _ptr(pr_))
            return _abi.PktSoa(_abi.AF_V4, _ptr(s_), _ptr(d_), None, None, None, _ptr(dp_), _ptr(pr_))
        flags = 0
        if force_linear:
            flags |= _abi.F_FORCE_LINEAR
        if timing:
            flags |= _abi.F_TIMING
        if accumulate:
            flags |= _abi.F_ACCUMULATE
        if dev:
            import torch
            flags |= _abi.F_DEVICE
            if verdict is None:
                flags |= _abi.F_NO_VERDICT
            if stream is None:
                stream = torch.cuda.current_stream()
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
            pk = soa(src, dst, dport, proto)
            self._check(_abi.lib().cls_classify(self.h, table.id, C.byref(pk), n, _ptr(verdict),
                                                _ptr(counters), flags, s))
            return verdict, counters
        adt = np.uint8 if v16 else np.uint32
        src = np.ascontiguousarray(src, adt)
        dst = np.ascontiguousarray(dst, adt)
        dport = np.ascontiguousarray(dport, np.uint16)
        proto = np.ascontiguousarray(proto, np.uint8)
        v = np.zeros(n, np.uint8) if verdict is None else verdict
        c = np.zeros(table.n_rules + 1, np.uint64) if counters is None else counters
        pk = soa(src, dst, dport, proto)
        self._check(_abi.lib().cls_classify(self.h, table.id, C.byref(pk), n, _ptr(v), _ptr(c),
                                            flags, None))
        return v, c

    def classify_rules(self, table: Table, src, dst, dport, proto, verdict=None, rules=None, stream=None):
        """Each packet's ACLAction and terminating rule index (R: the default
        DENY) -- cls_classify_rules, the batch form of the matched rule
        evalACL logs; no counters.  numpy inputs: synchronous, returns
        (verdict uint8[n], rules uint32[n]); torch device tensors: enqueued on
        ``stream``, ``rules`` (int32[n]) and ``verdict`` (uint8[n], optional)
        written and returned."""
        n = int(len(dport))
        dev = _is_torch(src)
        v16 = (src.dim() if dev else np.ndim(src)) == 2

        def soa(s_, d_, dp_, pr_):
            if v16:
                return _abi.PktSoa(_abi.AF_V16, None, None, _ptr(s_), _ptr(d_), None, _ptr(dp_), _ptr(pr_))
            return _abi.PktSoa(_abi.AF_V4, _ptr(s_), _ptr(d_), None, None, None, _ptr(dp_), _ptr(pr_))
        if dev:
            import torch
            if stream is None:
                stream = torch.cuda.current_stream()
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
            if rules is None:
                rules = torch.empty(n, dtype=torch.int32, device=src.device)
            pk = soa(src, dst, dport, proto)
            self._check(_abi.lib().cls_classify_rules(self.h, table.id, C.byref(pk), n, _ptr(verdict),
                                                      _ptr(rules), _abi.F_DEVICE, s))
            return verdict, rules
        adt = np.uint8 if v16 else np.uint32
        src = np.ascontiguousarray(src, adt)
        dst = np.ascontiguousarray(dst, adt)
        dport = np.ascontiguousarray(dport, np.uint16)
        proto = np.ascontiguousarray(proto, np.uint8)
        v = np.zeros(n, np.uint8) if verdict is None else verdict
        r = np.zeros(n, np.uint32) if rules is None else rules
        pk = soa(src, dst, dport, proto)
        self._check(_abi.lib().cls_classify_rules(self.h, table.id, C.byref(pk), n, _ptr(v), _ptr(r), 0, None))
        return v, r

    def stream_floor(self, src, dst, dport, proto, verdict, reps: int = 10, stream=None) -> float:
        """Average ms of the classify kernel's packet stream alone (same loads,
        stores and grid, no lookups) over a device batch: the measured floor
        the classify kernel is compared against (bench.py) -- the fastest
        stream shape."""
        return min(self.stream_floor_shapes(src, dst, dport, proto, verdict, reps, stream))

    def stream_floor_shapes(self, src, dst, dport, proto, verdict, reps: int = 10, stream=None):
        """Each stream shape's average ms (cls_stream_floor_shapes): index =
        variant << 1 | two workgroups per CU; IPv4 8 shapes, 16-byte 2."""
        import torch
        v16 = src.dim() == 2
        n = int(dport.numel())
        if v16:
            pk = _abi.PktSoa(_abi.AF_V16, None, None, _ptr(src), _ptr(dst), None, _ptr(dport), _ptr(proto))
            n -= n % 256
        else:
            pk = _abi.PktSoa(_abi.AF_V4, _ptr(src), _ptr(dst), None, None, None, _ptr(dport), _ptr(proto))
            n -= n % 4
        if stream is None:
            stream = torch.cuda.current_stream()
        s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        ms = (C.c_float * 8)()
        cnt = C.c_uint32(0)
        self._check(_abi.lib().cls_stream_floor_shapes(self.h, C.byref(pk), n, _ptr(verdict), reps, ms, 8,
                                                       C.byref(cnt), s))
        scale = int(dport.numel()) / n if n else 1.0
        return [ms[i] * scale for i in range(cnt.value)]

    def last_kernel_ms(self) -> float:
        ms = C.c_float(0)
        self._check(_abi.lib().cls_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def _timed(self, fn):
        n = C.c_uint32(0)
        self._check(fn(self.h, None, 0, C.byref(n)))
        buf = (C.c_float * max(1, n.value))()
        self._check(fn(self.h, buf, n.value, C.byref(n)))
        return [buf[i] for i in range(n.value)]

    def kernel_times(self, reset: bool = True, starts: bool = False):
        """Durations (ms) of every kernel timed since the last reset; with
        `starts`, (durations, start times in ms after the first one's)."""
        out = self._timed(_abi.lib().cls_kernel_times)
        if starts:
            out = (out, self._timed(_abi.lib().cls_kernel_starts))
        if reset:
            self._check(_abi.lib().cls_kernel_times_reset(self.h))
        return out

    # -- traffic ------------------------------------------------------------
    def gen_traffic_v4(self, spec: dict, first: int, out: dict, stream=None):
        """Generate packets [first, first+n) of the synthetic stream into the
        device tensors of ``out`` (src, dst, sport, dport, proto)."""
        pods = np.ascontiguousarray(spec.get("pod_ips", []), np.uint32)
        da = np.ascontiguousarray(spec.get("dst_addrs", []), np.uint32)
        dl = np.ascontiguousarray(spec.get("dst_lens", []), np.uint8)
        ports = np.ascontiguousarray(spec.get("ports", []), np.uint16)
        ts = _abi.TrafficSpec(spec["seed"], spec.get("pct_pod_src", 60), spec.get("pct_rule_dst", 50),
                              spec.get("pct_table_port", 50), spec.get("pct_icmp", 0),
                              pods.ctypes.data, len(pods), da.ctypes.data, dl.ctypes.data, len(da),
                              ports.ctypes.data, len(ports))
        n = int(len(out["dport"]))
        s = None
        if stream is not None:
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        self._check(_abi.lib().cls_gen_traffic_v4(
            self.h, C.byref(ts), first, n, _ptr(out.get("src")), _ptr(out.get("dst")),
            _ptr(out.get("sport")), _ptr(out.get("dport")), _ptr(out.get("proto")), s))

    def gen_traffic_v16(self, spec: dict, first: int, out: dict, stream=None):
        """The 16-byte stream (cls_traffic_spec16) into device tensors: src,
        dst uint8[n, 16] (16-B aligned), sport, dport, proto.  Pools:
        pod_ips / dst_addrs uint8[m, 16], dst_lens 0..128, ports."""
        pods = np.ascontiguousarray(spec.get("pod_ips", np.zeros((0, 16))), np.uint8)
        da = np.ascontiguousarray(spec.get("dst_addrs", np.zeros((0, 16))), np.uint8)
        dl = np.ascontiguousarray(spec.get("dst_lens", []), np.uint8)
        ports = np.ascontiguousarray(spec.get("ports", []), np.uint16)
        ts = _abi.TrafficSpec16(spec["seed"], spec.get("pct_pod_src", 60), spec.get("pct_rule_dst", 50),
                                spec.get("pct_table_port", 50), spec.get("pct_icmp", 0),
                                pods.ctypes.data, len(pods), da.ctypes.data, dl.ctypes.data, len(da),
                                ports.ctypes.data, len(ports))
        n = int(len(out["dport"]))
        s = None
        if stream is not None:
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        self._check(_abi.lib().cls_gen_traffic_v16(
            self.h, C.byref(ts), first, n, _ptr(out.get("src")), _ptr(out.get("dst")),
            _ptr(out.get("sport")), _ptr(out.get("dport")), _ptr(out.get("proto")), s))

    # -- ACL configuration (ACLConfig) ---------------------------------------
    def acl_put(self, name: str, rules, ingress, egress):
        cr = _abi.CRules(rules)
        ing = (C.c_char_p * max(1, len(ingress)))(*[x.encode() for x in ingress])
        eg = (C.c_char_p * max(1, len(egress)))(*[x.encode() for x in egress])
        return _abi.lib().cls_acl_put(self.h, name.encode(), cr.ptr(), cr.n, ing, len(ingress),
                                      eg, len(egress))

    def acl_del(self, name: str):
        return _abi.lib().cls_acl_del(self.h, name.encode())

    def acl_table(self, name: str) -> int:
        t = C.c_uint32(0)
        rc = _abi.lib().cls_acl_table(self.h, name.encode(), C.byref(t))
        return int(t.value) if rc == 0 else -1

    def acl_counts(self):
        a, c = C.c_uint32(0), C.c_uint32(0)
        self._check(_abi.lib().cls_acl_counts(self.h, C.byref(a), C.byref(c)))
        return a.value, c.value

    def acl_stats(self):
        """(tables compiled, puts that kept the installed table) by cls_acl_put."""
        a, c = C.c_uint32(0), C.c_uint32(0)
        self._check(_abi.lib().cls_acl_stats(self.h, C.byref(a), C.byref(c)))
        return a.value, c.value

    def if_id(self, name: str) -> int:
        i = C.c_uint32(0)
        self._check(_abi.lib().cls_if_id(self.h, name.encode(), C.byref(i)))
        return i.value

    def if_acls(self, if_id: int):
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(_abi.lib().cls_if_acls(self.h, if_id, C.byref(a), C.byref(b)))
        return a.value, b.value

    def connect_batch(self, src_if, dst_if, src, dst, proto, sport, dport, mode: str = "auto",
                      count: bool = False, out=None) -> np.ndarray:
        """testConnection over a batch (cls_connect_batch).  Addresses: host-order
        u32 (IPv4) or n x 16 network-order bytes (IPv6, IPv4-mapped = IPv4).
        mode: "auto" (ACLs with a classifier image use it for batches >=
        65536), "classifier" (at any size) or "linear" (every ACL scanned).
        count: add every evalACL call's terminating rule to the tables'
        connection counters (conn_counters).  out (device batches): a
        contiguous uint8 GPU tensor of n verdicts to write instead of a new
        one."""
        flags = {"auto": 0, "classifier": _abi.F_CONN_CLS, "linear": _abi.F_FORCE_LINEAR}[mode]
        if count:
            flags |= _abi.F_COUNT
        if _is_torch(src):
            return self._connect_batch_device(src_if, dst_if, src, dst, proto, sport, dport, flags, out)
        v16 = np.asarray(src).ndim == 2
        if v16:
            s = np.ascontiguousarray(src, np.uint8).reshape(-1, 16)
            d = np.ascontiguousarray(dst, np.uint8).reshape(-1, 16)
        else:
            s, d = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(dst, np.uint32)
        si, di = np.ascontiguousarray(src_if, np.uint32), np.ascontiguousarray(dst_if, np.uint32)
        p, sp = np.ascontiguousarray(proto, np.uint8), np.ascontiguousarray(sport, np.uint16)
        dp = np.ascontiguousarray(dport, np.uint16)
        n = len(s)
        out = np.zeros(n, np.uint8)
        if v16:
            pk = _abi.PktSoa(_abi.AF_V16, None, None, _ptr(s), _ptr(d), _ptr(sp), _ptr(dp), _ptr(p))
        else:
            pk = _abi.PktSoa(_abi.AF_V4, _ptr(s), _ptr(d), None, None, _ptr(sp), _ptr(dp), _ptr(p))
        cs = _abi.ConnSoa(pk, _ptr(si), _ptr(di))
        self._check(_abi.lib().cls_connect_batch(self.h, C.byref(cs), n, _ptr(out), flags, None))
        return out

    def _connect_batch_device(self, src_if, dst_if, src, dst, proto, sport, dport, flags, out=None):
        """Device-resident batch (CLS_F_DEVICE): contiguous GPU tensors of 4-byte
        interface ids, 4-byte (or n x 16 uint8) addresses, 2-byte ports and
        1-byte protocols, already written (the call runs on the engine's
        stream).  Returns a uint8 tensor (`out` when given)."""
        import torch
        v16 = src.dim() == 2
        arrs = (src_if, dst_if, src, dst, sport, dport, proto)
        sizes = (4, 4, 1 if v16 else 4, 1 if v16 else 4, 2, 2, 1)
        n = src.shape[0]
        for x, sz in zip(arrs, sizes):
            if not (_is_torch(x) and x.is_cuda and x.is_contiguous() and x.element_size() == sz and x.shape[0] == n):
                raise ClsError("device connection batch: contiguous GPU tensors of element sizes %s" % (sizes,))
        if out is None:
            out = torch.empty(n, dtype=torch.uint8, device=src.device)
        elif not (_is_torch(out) and out.is_cuda and out.is_contiguous() and out.element_size() == 1 and
                  out.shape[0] == n):
            raise ClsError("device connection batch: out must be a contiguous uint8 GPU tensor of n elements")
        if v16:
            pk = _abi.PktSoa(_abi.AF_V16, None, None, _ptr(src), _ptr(dst), _ptr(sport), _ptr(dport), _ptr(proto))
        else:
            pk = _abi.PktSoa(_abi.AF_V4, _ptr(src), _ptr(dst), None, None, _ptr(sport), _ptr(dport), _ptr(proto))
        cs = _abi.ConnSoa(pk, _ptr(src_if), _ptr(dst_if))
        self._check(_abi.lib().cls_connect_batch(self.h, C.byref(cs), n, _ptr(out), flags | _abi.F_DEVICE, None))
        return out

    def connect_rules(self, src_if, dst_if, src, dst, proto, sport, dport, mode: str = "auto", out=None,
                      rules_out=None, stream=None):
        """connect_batch with the trace (cls_connect_rules): the ConnectionAction
        of every connection and the terminating rule of each of its four
        evalACL calls, in testConnection's order (SYN src inbound, SYN dst
        outbound, SYN-ACK dst inbound, SYN-ACK src outbound): the index in
        that ACL's table, R for the default DENY, -1 for a call not made or on
        a nil ACL.  The tables are the interfaces' bindings at the call
        (if_acls).  No counters.  Host arrays: (verdict uint8[n], rules
        int32[n, 4]).  Torch device tensors: the same as GPU tensors (``out``
        uint8[n] / ``rules_out`` int32[n, 4], contiguous, when given),
        enqueued on ``stream`` (default: the engine's)."""
        flags = {"auto": 0, "classifier": _abi.F_CONN_CLS, "linear": _abi.F_FORCE_LINEAR}[mode]
        fn = _abi.lib().cls_connect_rules
        if _is_torch(src):
            import torch
            v16 = src.dim() == 2
            arrs = (src_if, dst_if, src, dst, sport, dport, proto)
            sizes = (4, 4, 1 if v16 else 4, 1 if v16 else 4, 2, 2, 1)
            n = src.shape[0]
            for x, sz in zip(arrs, sizes):
                if not (_is_torch(x) and x.is_cuda and x.is_contiguous() and x.element_size() == sz and
                        x.shape[0] == n):
                    raise ClsError("device connection batch: contiguous GPU tensors of element sizes %s" % (sizes,))
            if out is None:
                out = torch.empty(n, dtype=torch.uint8, device=src.device)
            elif not (_is_torch(out) and out.is_cuda and out.is_contiguous() and out.element_size() == 1 and
                      out.shape[0] == n):
                raise ClsError("device connection batch: out must be a contiguous uint8 GPU tensor of n elements")
            if rules_out is None:
                rules_out = torch.empty((n, 4), dtype=torch.int32, device=src.device)
            elif not (_is_torch(rules_out) and rules_out.is_cuda and rules_out.is_contiguous() and
                      rules_out.dtype == torch.int32 and tuple(rules_out.shape) == (n, 4) and
                      rules_out.data_ptr() % 16 == 0):
                raise ClsError("device connection trace: rules_out must be a contiguous, 16-byte aligned int32 "
                               "GPU tensor of shape (n, 4)")
            s = None
            if stream is not None:
                s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
            if v16:
                pk = _abi.PktSoa(_abi.AF_V16, None, None, _ptr(src), _ptr(dst), _ptr(sport), _ptr(dport), _ptr(proto))
            else:
                pk = _abi.PktSoa(_abi.AF_V4, _ptr(src), _ptr(dst), None, None, _ptr(sport), _ptr(dport), _ptr(proto))
            cs = _abi.ConnSoa(pk, _ptr(src_if), _ptr(dst_if))
            self._check(fn(self.h, C.byref(cs), n, _ptr(out), _ptr(rules_out), flags | _abi.F_DEVICE, s))
            return out, rules_out
        v16 = np.asarray(src).ndim == 2
        if v16:
            s = np.ascontiguousarray(src, np.uint8).reshape(-1, 16)
            d = np.ascontiguousarray(dst, np.uint8).reshape(-1, 16)
        else:
            s, d = np.ascontiguousarray(src, np.uint32), np.ascontiguousarray(dst, np.uint32)
        si, di = np.ascontiguousarray(src_if, np.uint32), np.ascontiguousarray(dst_if, np.uint32)
        p, sp = np.ascontiguousarray(proto, np.uint8), np.ascontiguousarray(sport, np.uint16)
        dp = np.ascontiguousarray(dport, np.uint16)
        n = len(s)
        v = np.zeros(n, np.uint8)
        r = np.full((max(n, 1), 4), -1, np.int32)[:n]       # (a valid pointer for n = 0)
        if v16:
            pk = _abi.PktSoa(_abi.AF_V16, None, None, _ptr(s), _ptr(d), _ptr(sp), _ptr(dp), _ptr(p))
        else:
            pk = _abi.PktSoa(_abi.AF_V4, _ptr(s), _ptr(d), None, None, _ptr(sp), _ptr(dp), _ptr(p))
        cs = _abi.ConnSoa(pk, _ptr(si), _ptr(di))
        self._check(fn(self.h, C.byref(cs), n, _ptr(v), _ptr(r), flags, None))
        return v, r

    def reach_matrix(self, if_ids, addrs, protos, sports, dports, mode: str = "auto", count: bool = False,
                     verdicts: bool = True, hist: bool = True, allow: bool = True, out=None, stream=None):
        """The reachability matrix (cls_reach_matrix): testConnection over every
        (probe, source, destination) cell of N endpoints -- ``if_ids`` (N,)
        and ``addrs`` (N,) host-order u32 or (N, 16) network-order bytes -- and
        P probes (``protos``, ``sports``, ``dports``), evaluated on the device
        from these lists alone.  Returns (verdicts [P, N, N] u8 | None, hist
        [P, 4] u64 | None: cells per ConnectionAction, allow [P, N] u32 | None:
        per (probe, source) the destinations it reaches); ``verdicts`` /
        ``hist`` / ``allow`` False leaves one out (not all three).  mode and
        count: as connect_batch.  The inputs are always host arrays.  out:
        None for numpy results (the call returns with them), or a sequence
        (verdicts, hist, allow) of contiguous torch GPU tensors -- u8
        [P, N, N], 8-byte [P, 4], 4-byte [P, N]; None for a wanted one
        allocates it -- which selects the device form: the call only enqueues
        on ``stream`` (default: the engine's) and returns the tensors."""
        flags = {"auto": 0, "classifier": _abi.F_CONN_CLS, "linear": _abi.F_FORCE_LINEAR}[mode]
        if count:
            flags |= _abi.F_COUNT
        if not verdicts:
            flags |= _abi.F_NO_VERDICT
        ids = np.ascontiguousarray(if_ids, np.uint32)
        a = np.asarray(addrs)
        v16 = a.ndim == 2
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 16) if v16 else np.ascontiguousarray(a, np.uint32)
        pr, sp = np.ascontiguousarray(protos, np.uint8), np.ascontiguousarray(sports, np.uint16)
        dp = np.ascontiguousarray(dports, np.uint16)
        n, p = len(ids), len(pr)
        if len(a) != n or len(sp) != p or len(dp) != p:
            raise ClsError("reach matrix: N interface ids and addresses, P protocols and ports")
        spec = _abi.ReachSpec(_abi.AF_V16 if v16 else _abi.AF_V4, n, _ptr(ids), None if v16 else _ptr(a),
                              _ptr(a) if v16 else None, p, _ptr(pr), _ptr(sp), _ptr(dp))
        want = (verdicts, hist, allow)
        shapes = ((p, n, n), (p, 4), (p, n))
        if out is None:
            res = [np.zeros(sh, dt) if w else None for w, sh, dt in zip(want, shapes, (np.uint8, np.uint64, np.uint32))]
            s = None
        else:
            import torch
            flags |= _abi.F_DEVICE
            res = list(out)
            if len(res) != 3:
                raise ClsError("reach matrix: out is (verdicts, hist, allow)")
            for k, (w, sh, dt, sz) in enumerate(zip(want, shapes, (torch.uint8, torch.int64, torch.int32), (1, 8, 4))):
                if not w:
                    res[k] = None
                elif res[k] is None:
                    res[k] = torch.empty(sh, dtype=dt, device="cuda")
                elif not (_is_torch(res[k]) and res[k].is_cuda and res[k].is_contiguous() and
                          res[k].element_size() == sz and tuple(res[k].shape) == sh):
                    raise ClsError("reach matrix: out[%d] must be a contiguous GPU tensor of shape %s, %d-byte "
                                   "elements" % (k, sh, sz))
            s = None
            if stream is not None:
                s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        self._check(_abi.lib().cls_reach_matrix(self.h, C.byref(spec), _ptr(res[0]), _ptr(res[1]), _ptr(res[2]),
                                                flags, s))
        return tuple(res)

    def reach_diff(self, if_ids, addrs, protos, sports, dports, base, cap=None, mode: str = "auto",
                   count: bool = False, verdicts: bool = True, hist: bool = False, allow: bool = False,
                   trans: bool = True, changed: bool = True, inplace: bool = False, out=None, stream=None):
        """The reachability matrix of reach_matrix's arguments against a
        baseline (cls_reach_diff): ``base`` is the [P, N, N] u8 matrix of an
        earlier call, compared on the device.  Returns ReachDiff(verdicts
        [P, N, N] u8: the new matrix, changes: the changed cells in cell
        order, n_changes: all of them, also beyond ``cap``, trans [P, 4, 4]
        u64: cells per (base & 3, new), changed [P, N] u32: changed cells per
        (probe, source), hist, allow: as reach_matrix); what is not wanted is
        None.  ``cap``: the records kept (None: P N^2, or the rows of the
        caller's ``changes`` tensor); 0: no records, and n_changes only when
        neither trans nor changed is wanted.  ``inplace``: the new matrix
        replaces ``base`` (returned as verdicts).  A numpy ``base`` selects
        the host form: the call returns with numpy results, changes a
        structured array (_abi.REACH_CHANGE) cut to min(n_changes, cap) and
        n_changes an int.  A torch GPU uint8 ``base`` selects the device form:
        changes is an int32 [cap, 4] tensor of (probe, src, dst, was | now <<
        8) rows, of which the first min(n_changes, cap) are written,
        n_changes an int64 [1] tensor; ``out``, a ReachDiff or a sequence in
        its order, gives the caller's tensors (None for a wanted one
        allocates it), and the call only enqueues on ``stream`` (default: the
        engine's)."""
        flags = {"auto": 0, "classifier": _abi.F_CONN_CLS, "linear": _abi.F_FORCE_LINEAR}[mode]
        if count:
            flags |= _abi.F_COUNT
        if not (verdicts or inplace):
            flags |= _abi.F_NO_VERDICT
        ids = np.ascontiguousarray(if_ids, np.uint32)
        a = np.asarray(addrs)
        v16 = a.ndim == 2
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 16) if v16 else np.ascontiguousarray(a, np.uint32)
        pr, sp = np.ascontiguousarray(protos, np.uint8), np.ascontiguousarray(sports, np.uint16)
        dp = np.ascontiguousarray(dports, np.uint16)
        n, p = len(ids), len(pr)
        if len(a) != n or len(sp) != p or len(dp) != p:
            raise ClsError("reach diff: N interface ids and addresses, P protocols and ports")
        spec = _abi.ReachSpec(_abi.AF_V16 if v16 else _abi.AF_V4, n, _ptr(ids), None if v16 else _ptr(a),
                              _ptr(a) if v16 else None, p, _ptr(pr), _ptr(sp), _ptr(dp))
        dev = _is_torch(base)
        given = [None] * 7 if out is None else list(out)
        if len(given) != 7 or (not dev and out is not None):
            raise ClsError("reach diff: out is a ReachDiff of GPU tensors, for a GPU base")
        if cap is None:
            cap = given[1].shape[0] if given[1] is not None else p * n * n
        cap = int(cap)
        listed = cap > 0 or not (trans or changed)
        # (verdicts, changes, n_changes, trans, changed, hist, allow): wanted, shape
        want = (verdicts and not inplace, cap > 0, listed, trans, changed, hist, allow)
        shapes = ((p, n, n), (cap, 4), (1,), (p, 4, 4), (p, n), (p, 4), (p, n))
        if dev:
            import torch
            flags |= _abi.F_DEVICE
            if not (base.is_cuda and base.is_contiguous() and base.dtype == torch.uint8 and
                    tuple(base.shape) == (p, n, n)):
                raise ClsError("reach diff: base must be a contiguous uint8 GPU tensor of shape (P, N, N)")
            kinds = ((torch.uint8, 1), (torch.int32, 4), (torch.int64, 8), (torch.int64, 8), (torch.int32, 4),
                     (torch.int64, 8), (torch.int32, 4))
            res = []
            for k, (w, sh, (dt, sz)) in enumerate(zip(want, shapes, kinds)):
                t = given[k] if w else None
                if w and t is None:
                    t = torch.empty(sh, dtype=dt, device=base.device)
                elif w and not (_is_torch(t) and t.is_cuda and t.is_contiguous() and t.element_size() == sz and
                                tuple(t.shape) == sh):
                    raise ClsError("reach diff: out.%s must be a contiguous GPU tensor of shape %s, %d-byte elements"
                                   % (ReachDiff._fields[k], sh, sz))
                res.append(t)
            s = None
            if stream is not None:
                s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        else:
            base = np.asarray(base)
            if not (base.dtype == np.uint8 and base.shape == (p, n, n) and base.flags.c_contiguous and
                    (base.flags.writeable or not inplace)):
                raise ClsError("reach diff: base must be a contiguous uint8 array of shape (P, N, N)")
            kinds = (np.uint8, np.int32, np.uint64, np.uint64, np.uint32, np.uint64, np.uint32)
            res = [np.zeros(sh, dt) if w else None for w, sh, dt in zip(want, shapes, kinds)]
            if res[1] is not None:
                res[1] = np.zeros(min(cap, p * n * n), _abi.REACH_CHANGE)
            s = None
        if inplace:
            res[0] = base
        o = _abi.ReachDiffOut(_ptr(res[0]), _ptr(res[5]), _ptr(res[6]), _ptr(res[1]), cap if res[1] is not None else 0,
                              _ptr(res[2]), _ptr(res[3]), _ptr(res[4]))
        self._check(_abi.lib().cls_reach_diff(self.h, C.byref(spec), _ptr(base), C.byref(o), flags, s))
        if not dev and res[2] is not None:
            res[2] = int(res[2][0])
            if res[1] is not None:
                res[1] = res[1][:min(res[2], cap)]
        return ReachDiff(*res)

    @staticmethod
    def port_classes(rules, proto: int) -> np.ndarray:
        """The port class starts of one rule list for ``proto``
        (cls_port_classes; no device): ascending u16, the first 0 -- 0 and
        the lo16 / hi16 + 1 of the rules that test the destination port."""
        cr = rules if isinstance(rules, _abi.CRules) else _abi.CRules(rules)
        n = C.c_uint32(0)
        rc = _abi.lib().cls_port_classes(cr.ptr(), cr.n, proto, None, 0, C.byref(n))
        if rc != 0:
            raise ClsError("cls_port_classes: rc=%d" % rc)
        lo = np.zeros(n.value, np.uint16)
        rc = _abi.lib().cls_port_classes(cr.ptr(), cr.n, proto, _ptr(lo), n.value, C.byref(n))
        if rc != 0:
            raise ClsError("cls_port_classes: rc=%d" % rc)
        return lo

    def reach_ports(self, if_ids, addrs, proto: int, sport: int, cap=None, mode: str = "auto", out=None,
                    stream=None):
        """The port sweep (cls_reach_ports): on which destination ports, of
        all 65,536, endpoint s reaches endpoint d -- ``if_ids`` and ``addrs``
        as reach_matrix, one ``proto`` and ``sport``.  Returns
        ReachPorts(ranges: the maximal (src, dst, port_lo, port_hi, action)
        ranges in (src, dst, port_lo) order, n_ranges: all of them, also
        beyond ``cap``, runs [N, N] u32: ranges per pair, allow_ports [N, N]
        u32: dports with CONN_ALLOW, hist [4] u64: (pair, dport) cells per
        ConnectionAction, n_classes: the port classes K evaluated per pair).
        out None: the host form -- numpy results, ranges a structured array
        (_abi.PORT_RANGE) cut to min(n_ranges, cap), n_ranges an int; cap None
        keeps all ranges (a first call counts them), cap 0 asks for none.
        out a sequence (ranges, n_ranges, runs, allow_ports, hist) of
        contiguous torch GPU tensors (None allocates one): the device form --
        ranges an int32 [cap, 4] tensor of (src, dst, port_lo | port_hi << 16,
        action) rows of which the first min(n_ranges, cap) are written (cap
        None: its rows), n_ranges int64 [1]; the call only enqueues on
        ``stream`` (default: the engine's).  n_classes is an int either way."""
        flags = {"auto": 0, "classifier": _abi.F_CONN_CLS, "linear": _abi.F_FORCE_LINEAR}[mode]
        ids = np.ascontiguousarray(if_ids, np.uint32)
        a = np.asarray(addrs)
        v16 = a.ndim == 2
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 16) if v16 else np.ascontiguousarray(a, np.uint32)
        n = len(ids)
        if len(a) != n:
            raise ClsError("reach ports: N interface ids and addresses")
        pr, sp = np.array([proto], np.uint8), np.array([sport], np.uint16)
        spec = _abi.ReachSpec(_abi.AF_V16 if v16 else _abi.AF_V4, n, _ptr(ids), None if v16 else _ptr(a),
                              _ptr(a) if v16 else None, 1, _ptr(pr), _ptr(sp), None)
        k = np.zeros(1, np.uint32)
        fn = _abi.lib().cls_reach_ports
        if out is None:
            total = np.zeros(1, np.uint64)
            if cap is None:
                o = _abi.ReachPortsOut(None, 0, _ptr(total), None, None, None, _ptr(k))
                self._check(fn(self.h, C.byref(spec), C.byref(o), flags, None))
                cap = int(total[0])
            cap = int(cap)
            rec = np.zeros(cap, _abi.PORT_RANGE) if cap > 0 else None
            runs, allow = np.zeros((n, n), np.uint32), np.zeros((n, n), np.uint32)
            hist = np.zeros(4, np.uint64)
            o = _abi.ReachPortsOut(_ptr(rec), cap, _ptr(total), _ptr(runs), _ptr(allow), _ptr(hist), _ptr(k))
            self._check(fn(self.h, C.byref(spec), C.byref(o), flags, None))
            if rec is not None:
                rec = rec[:min(int(total[0]), cap)]
            return ReachPorts(rec, int(total[0]), runs, allow, hist, int(k[0]))
        import torch
        res = list(out)
        if len(res) != 5:
            raise ClsError("reach ports: out is (ranges, n_ranges, runs, allow_ports, hist)")
        if cap is None:
            if res[0] is None:
                raise ClsError("reach ports: the device form needs cap or a ranges tensor")
            cap = res[0].shape[0]
        cap = int(cap)
        shapes = ((cap, 4), (1,), (n, n), (n, n), (4,))
        kinds = ((torch.int32, 4), (torch.int64, 8), (torch.int32, 4), (torch.int32, 4), (torch.int64, 8))
        for i, (sh, (dt, sz)) in enumerate(zip(shapes, kinds)):
            if i == 0 and cap == 0:
                res[0] = None
            elif res[i] is None:
                res[i] = torch.empty(sh, dtype=dt, device="cuda")
            elif not (_is_torch(res[i]) and res[i].is_cuda and res[i].is_contiguous() and
                      res[i].element_size() == sz and tuple(res[i].shape) == sh):
                raise ClsError("reach ports: out[%d] must be a contiguous GPU tensor of shape %s, %d-byte elements"
                               % (i, sh, sz))
        s = None
        if stream is not None:
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        o = _abi.ReachPortsOut(_ptr(res[0]), cap, _ptr(res[1]), _ptr(res[2]), _ptr(res[3]), _ptr(res[4]), _ptr(k))
        self._check(fn(self.h, C.byref(spec), C.byref(o), flags | _abi.F_DEVICE, s))
        return ReachPorts(*res, int(k[0]))

    @staticmethod
    def addr_classes(rules) -> np.ndarray:
        """The IPv4 address class starts of one rule list (cls_addr_classes;
        no device): ascending u32, the first 0 -- 0 and the lo / hi + 1 of the
        source and destination networks whose effective family is 4."""
        cr = rules if isinstance(rules, _abi.CRules) else _abi.CRules(rules)
        n = C.c_uint32(0)
        rc = _abi.lib().cls_addr_classes(cr.ptr(), cr.n, None, 0, C.byref(n))
        if rc != 0:
            raise ClsError("cls_addr_classes: rc=%d" % rc)
        lo = np.zeros(n.value, np.uint32)
        rc = _abi.lib().cls_addr_classes(cr.ptr(), cr.n, _ptr(lo), n.value, C.byref(n))
        if rc != 0:
            raise ClsError("cls_addr_classes: rc=%d" % rc)
        return lo

    @staticmethod
    def cover_classes(rules, side: int) -> np.ndarray:
        """The IPv4 address class starts of one side of a rule list
        (cls_cover_classes; no device): side 0 the source networks, 1 the
        destination networks; ascending u32, the first 0."""
        cr = rules if isinstance(rules, _abi.CRules) else _abi.CRules(rules)
        n = C.c_uint32(0)
        rc = _abi.lib().cls_cover_classes(cr.ptr(), cr.n, int(side), None, 0, C.byref(n))
        if rc != 0:
            raise ClsError("cls_cover_classes: rc=%d" % rc)
        lo = np.zeros(n.value, np.uint32)
        rc = _abi.lib().cls_cover_classes(cr.ptr(), cr.n, int(side), _ptr(lo), n.value, C.byref(n))
        if rc != 0:
            raise ClsError("cls_cover_classes: rc=%d" % rc)
        return lo

    def table_cover(self, table, af: int = 4, mode: str = "auto", out=None, stream=None):
        """The rule coverage sweep (cls_table_cover) of one table over the whole
        IPv4 packet space (``af`` 16: the same packets as ::ffff:a in the
        16-byte layout): which rules no packet terminates at, and the least
        packet in (src, dst, proto, dport) order that terminates at each of
        the others.  Returns a dict: live uint8 [R+1] (index R: the default
        DENY), witness [R+1] (_abi.COVER_WITNESS: src, dst, dport, proto --
        3 standing for every protocol above 2 --, live; zeros for a dead
        rule), cells uint64 [R+1] (cells of the class product terminating at
        the rule; sums to n_cells), n_dead (rules below R that are dead),
        n_cells (Ks Kd T) and dims (Ks, Kd, Kt, Ku).  mode "linear": the
        linear kernel evaluates.
        out None: the host form -- numpy results, n_dead an int.
        out a sequence (live, witness, cells, n_dead) of contiguous torch GPU
        tensors (None allocates one): the device form -- live uint8 [R+1],
        witness int32 [R+1, 4] rows of (src, dst, dport | proto << 16 | live
        << 24, 0), cells int64 [R+1], n_dead int32 [1]; the call only enqueues
        on ``stream`` (default: the engine's).  n_cells and dims are host
        values either way."""
        flags = {"auto": 0, "linear": _abi.F_FORCE_LINEAR}[mode]
        tid = table.id if isinstance(table, Table) else int(table)
        r = (table.n_rules if isinstance(table, Table) else self._table_rules(tid)) + 1
        n_cells, dims = np.zeros(1, np.uint64), np.zeros(4, np.uint32)
        fn = _abi.lib().cls_table_cover
        names = ("live", "witness", "cells", "n_dead")
        if out is None:
            live, wit = np.zeros(r, np.uint8), np.zeros(r, _abi.COVER_WITNESS)
            cells, dead = np.zeros(r, np.uint64), np.zeros(1, np.uint32)
            o = _abi.CoverOut(_ptr(live), _ptr(wit), _ptr(cells), _ptr(dead), _ptr(n_cells), _ptr(dims))
            self._check(fn(self.h, tid, int(af), C.byref(o), flags, None))
            return dict(zip(names, (live, wit, cells, int(dead[0]))), n_cells=int(n_cells[0]),
                        dims=tuple(int(x) for x in dims))
        import torch
        res = list(out)
        if len(res) != 4:
            raise ClsError("table cover: out is (live, witness, cells, n_dead)")
        shapes = ((r,), (r, 4), (r,), (1,))
        kinds = ((torch.uint8, 1), (torch.int32, 4), (torch.int64, 8), (torch.int32, 4))
        for i, (sh, (dt, sz)) in enumerate(zip(shapes, kinds)):
            if res[i] is None:
                res[i] = torch.empty(sh, dtype=dt, device="cuda")
            elif not (_is_torch(res[i]) and res[i].is_cuda and res[i].is_contiguous() and
                      res[i].element_size() == sz and tuple(res[i].shape) == sh):
                raise ClsError("table cover: out[%d] must be a contiguous GPU tensor of shape %s, %d-byte "
                               "elements" % (i, sh, sz))
        s = None
        if stream is not None:
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        o = _abi.CoverOut(_ptr(res[0]), _ptr(res[1]), _ptr(res[2]), _ptr(res[3]), _ptr(n_cells), _ptr(dims))
        self._check(fn(self.h, tid, int(af), C.byref(o), flags | _abi.F_DEVICE, s))
        return dict(zip(names, res), n_cells=int(n_cells[0]), dims=tuple(int(x) for x in dims))

    def table_diff(self, ta, tb, af: int = 4, mode: str = "auto", rec_cap: int = 1 << 20, out=None, stream=None):
        """The table diff (cls_table_diff): the packets of the whole IPv4
        packet space (``af`` 16: the same packets as ::ffff:a in the 16-byte
        layout) whose ACLAction differs between table ``ta`` and table ``tb``,
        over the joint classes of the two rule lists -- cover_classes and
        port_classes of a's rules followed by b's.  Returns a dict: equal
        (n_diff == 0), n_diff, pairs uint64 [4, 4] (cells per (was, now); sums
        to n_cells), first (_abi.COVER_WITNESS: the least differing packet,
        live 0 if none), cells_a uint64 [Ra+1] and wit_a [Ra+1] (differing
        cells terminating at rule k of a and the least such packet; index Ra:
        the default DENY), cells_b, wit_b [Rb+1], records (_abi.TDIFF_REC, one
        per maximal run of differing cells of one row and protocol with equal
        (was, now, rule_a, rule_b), ascending; the first min(rec_cap, n_rec)),
        n_rec (all of them), n_cells and dims (the joint Ks, Kd, Kt, Ku).
        mode "linear": the linear kernel evaluates.
        out None: the host form -- numpy results, the counts ints.
        out a sequence (n_diff, pairs, first, cells_a, wit_a, cells_b, wit_b,
        records, n_rec) of contiguous torch GPU tensors (None allocates one):
        the device form -- n_diff int64 [1], pairs int64 [4, 4], first int32
        [1, 4] and wit_a / wit_b int32 [R+1, 4] rows of (src, dst, dport |
        proto << 16 | live << 24, 0), cells_a / cells_b int64 [R+1], records
        int32 [rec_cap, 8], n_rec int64 [1]; the call only enqueues on
        ``stream`` (default: the engine's) and ``equal`` is None.  n_cells and
        dims are host values either way."""
        flags = {"auto": 0, "linear": _abi.F_FORCE_LINEAR}[mode]
        ids = [t.id if isinstance(t, Table) else int(t) for t in (ta, tb)]
        ra, rb = [(t.n_rules if isinstance(t, Table) else self._table_rules(i)) + 1 for t, i in zip((ta, tb), ids)]
        rec_cap = int(rec_cap)
        n_cells, dims = np.zeros(1, np.uint64), np.zeros(4, np.uint32)
        fn = _abi.lib().cls_table_diff
        names = ("n_diff", "pairs", "first", "cells_a", "wit_a", "cells_b", "wit_b", "records", "n_rec")
        if out is None:
            n_rec, cap = np.zeros(1, np.uint64), rec_cap
            res = [np.zeros(1, np.uint64), np.zeros((4, 4), np.uint64), np.zeros(1, _abi.COVER_WITNESS),
                   np.zeros(ra, np.uint64), np.zeros(ra, _abi.COVER_WITNESS), np.zeros(rb, np.uint64),
                   np.zeros(rb, _abi.COVER_WITNESS), np.zeros(cap, _abi.TDIFF_REC), n_rec]
            o = _abi.TDiffOut(*[_ptr(a) for a in res[:7]], _ptr(res[7]) if cap else None, cap, _ptr(n_rec),
                              _ptr(n_cells), _ptr(dims))
            self._check(fn(self.h, ids[0], ids[1], int(af), C.byref(o), flags, None))
            r = dict(zip(names, res), n_cells=int(n_cells[0]), dims=tuple(int(x) for x in dims))
            r["n_diff"], r["n_rec"], r["first"] = int(res[0][0]), int(n_rec[0]), res[2][0]
            r["records"] = res[7][:min(cap, r["n_rec"])]
            r["equal"] = r["n_diff"] == 0
            return r
        import torch
        res = list(out)
        if len(res) != len(names):
            raise ClsError("table diff: out is (%s)" % ", ".join(names))
        shapes = ((1,), (4, 4), (1, 4), (ra,), (ra, 4), (rb,), (rb, 4), (rec_cap, 8), (1,))
        i64, i32 = (torch.int64, 8), (torch.int32, 4)
        kinds = (i64, i64, i32, i64, i32, i64, i32, i32, i64)
        for i, (sh, (dt, sz)) in enumerate(zip(shapes, kinds)):
            if res[i] is None:
                res[i] = torch.empty(sh, dtype=dt, device="cuda")
            elif not (_is_torch(res[i]) and res[i].is_cuda and res[i].is_contiguous() and
                      res[i].element_size() == sz and tuple(res[i].shape) == sh):
                raise ClsError("table diff: out[%d] must be a contiguous GPU tensor of shape %s, %d-byte "
                               "elements" % (i, sh, sz))
        s = None
        if stream is not None:
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        o = _abi.TDiffOut(*[_ptr(a) for a in res[:7]], _ptr(res[7]) if rec_cap else None, rec_cap, _ptr(res[8]),
                          _ptr(n_cells), _ptr(dims))
        self._check(fn(self.h, ids[0], ids[1], int(af), C.byref(o), flags | _abi.F_DEVICE, s))
        return dict(zip(names, res), equal=None, n_cells=int(n_cells[0]), dims=tuple(int(x) for x in dims))

    @staticmethod
    def _skip_mask(skip, r: int) -> np.ndarray:
        """``skip`` -- None, an iterable of rule indices, or the uint64
        bitmask itself -- as the (r + 63) // 64 words cls_table_need takes."""
        words = max(1, (r + 63) // 64)
        if isinstance(skip, np.ndarray) and skip.dtype == np.uint64:
            if len(skip) < (r + 63) // 64:
                raise ClsError("table need: skip has %d words, %d rules need %d" % (len(skip), r, (r + 63) // 64))
            return np.ascontiguousarray(skip)
        m = np.zeros(words, np.uint64)
        for k in (() if skip is None else skip):
            k = int(k)
            if not 0 <= k < r:
                raise ClsError("table need: skip names rule %d of %d" % (k, r))
            m[k >> 6] |= np.uint64(1 << (k & 63))
        return m

    @staticmethod
    def _need_result(res, n_cells, dims):
        names = ("need", "free", "first", "changed", "witness", "counts")
        return dict(zip(names, res), n_cells=int(n_cells[0]), dims=tuple(int(x) for x in dims))

    @staticmethod
    def table_need_host(rules, skip=None):
        """cls_table_need_host: table_need's host form computed without a
        device, in plain C++ over the same bit rows (the CPU baseline)."""
        cr = rules if isinstance(rules, _abi.CRules) else _abi.CRules(rules)
        r = cr.n
        m = Engine._skip_mask(skip, r)
        n_cells, dims = np.zeros(1, np.uint64), np.zeros(4, np.uint32)
        res = [np.zeros(r, np.uint8), np.zeros(r, np.uint8), np.zeros(r + 1, np.uint64), np.zeros(r, np.uint64),
               np.zeros(r, _abi.NEED_WITNESS), np.zeros(4, np.uint32)]
        o = _abi.NeedOut(*[_ptr(a) for a in res], _ptr(n_cells), _ptr(dims))
        rc = _abi.lib().cls_table_need_host(cr.ptr(), cr.n, _ptr(m), C.byref(o))
        if rc != 0:
            raise ClsError("cls_table_need_host: rc=%d" % rc)
        return Engine._need_result(res, n_cells, dims)

    def table_need(self, table, skip=None, out=None, stream=None):
        """The rule necessity sweep (cls_table_need) of one table over the
        whole IPv4 packet space: which rules the list can lose without
        changing any packet's ACLAction.  ``skip``: rules treated as deleted
        (indices, or the uint64 bitmask).  Returns a dict: need uint8 [R]
        (_abi.NEED_SKIPPED / NEED_DEAD / NEED_REDUNDANT / NEED_NEEDED), free
        uint8 [R] (1: deletable together with every other free rule), first
        uint64 [R+1] (cells whose first match is the rule; index R: the
        default DENY; sums to n_cells), changed uint64 [R] (cells whose action
        changes without the rule), witness [R] (_abi.NEED_WITNESS: for a
        NEEDED rule the least packet that changes, after = 0x80 | the action
        it gets without the rule, fall = the rule that takes it then; zeros
        otherwise), counts uint32 [4] (rules per need value), n_cells and dims
        (Ks, Kd, Kt, Ku).  Native IPv6 packets are out of scope: a rule with
        an IPv6 network is reported dead.
        out None: the host form -- numpy results.
        out a sequence (need, free, first, changed, witness, counts) of
        contiguous torch GPU tensors (None allocates one; False leaves that
        output out, which spares the second pass when it is free): the device
        form -- need and free uint8 [R], first int64 [R+1], changed int64 [R],
        witness int32 [R, 4] rows of (src, dst, dport | proto << 16 | after <<
        24, fall), counts int32 [4]; the call only enqueues on ``stream``
        (default: the engine's).  n_cells and dims are host values either way."""
        tid = table.id if isinstance(table, Table) else int(table)
        r = table.n_rules if isinstance(table, Table) else self._table_rules(tid)
        m = self._skip_mask(skip, r)
        n_cells, dims = np.zeros(1, np.uint64), np.zeros(4, np.uint32)
        fn = _abi.lib().cls_table_need
        if out is None:
            res = [np.zeros(r, np.uint8), np.zeros(r, np.uint8), np.zeros(r + 1, np.uint64), np.zeros(r, np.uint64),
                   np.zeros(r, _abi.NEED_WITNESS), np.zeros(4, np.uint32)]
            o = _abi.NeedOut(*[_ptr(a) for a in res], _ptr(n_cells), _ptr(dims))
            self._check(fn(self.h, tid, _ptr(m), C.byref(o), 0, None))
            return self._need_result(res, n_cells, dims)
        import torch
        res = list(out)
        if len(res) != 6:
            raise ClsError("table need: out is (need, free, first, changed, witness, counts)")
        shapes = ((r,), (r,), (r + 1,), (r,), (r, 4), (4,))
        kinds = ((torch.uint8, 1), (torch.uint8, 1), (torch.int64, 8), (torch.int64, 8), (torch.int32, 4),
                 (torch.int32, 4))
        for i, (sh, (dt, sz)) in enumerate(zip(shapes, kinds)):
            if res[i] is False:
                res[i] = None
            elif res[i] is None:
                res[i] = torch.empty(sh, dtype=dt, device="cuda")
            elif not (_is_torch(res[i]) and res[i].is_cuda and res[i].is_contiguous() and
                      res[i].element_size() == sz and tuple(res[i].shape) == sh):
                raise ClsError("table need: out[%d] must be a contiguous GPU tensor of shape %s, %d-byte "
                               "elements" % (i, sh, sz))
        s = None
        if stream is not None:
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        o = _abi.NeedOut(*[_ptr(a) for a in res], _ptr(n_cells), _ptr(dims))
        self._check(fn(self.h, tid, _ptr(m), C.byref(o), _abi.F_DEVICE, s))
        return self._need_result(res, n_cells, dims)

    def _table_rules(self, tid: int) -> int:
        inf = _abi.TableInfo()
        self._check(_abi.lib().cls_table_get_info(self.h, tid, C.byref(inf)))
        return int(inf.n_rules)

    def reach_external(self, if_ids, addrs, protos, sports, dports, ext_if: int, dirs=("egress", "ingress"),
                       cap=None, mode: str = "auto", out=None, stream=None):
        """The external sweep (cls_reach_external): which remote IPv4
        addresses, of all 2^32, endpoint s reaches ("egress") and which reach
        it ("ingress") through the node's output interface ``ext_if`` (an
        interface id) -- ``if_ids``, ``addrs`` and the P probes as
        reach_matrix; ``dirs`` names the D directions wanted, indexed egress
        before ingress.  Returns a dict: ranges, the maximal (src, probe, dir,
        action, addr_lo, addr_hi) ranges in (dir, probe, src, addr_lo) order;
        total, all of them, also beyond ``cap``; runs [D, P, N] u32, ranges
        per line; allow_addrs [D, P, N] u64, addresses with CONN_ALLOW; hist
        [D, P, 4] u64, addresses per ConnectionAction; n_classes, the address
        classes K evaluated per line.
        out None: the host form -- numpy results, ranges a structured array
        (_abi.ADDR_RANGE) cut to min(total, cap), total an int; cap None keeps
        all ranges (a first call counts them), cap 0 asks for none.
        out a sequence (ranges, total, runs, allow_addrs, hist) of contiguous
        torch GPU tensors (None allocates one): the device form -- ranges an
        int32 [cap, 4] tensor of (src, probe | dir << 16 | action << 24,
        addr_lo, addr_hi) rows of which the first min(total, cap) are written
        (cap None: its rows), total int64 [1], allow_addrs and hist int64; the
        call only enqueues on ``stream`` (default: the engine's).  n_classes
        is an int either way."""
        flags = {"auto": 0, "classifier": _abi.F_CONN_CLS, "linear": _abi.F_FORCE_LINEAR}[mode]
        bits = {"egress": _abi.EXT_EGRESS, "ingress": _abi.EXT_INGRESS}
        dmask = 0
        for x in ([dirs] if isinstance(dirs, str) else dirs):
            if x not in bits:
                raise ClsError("reach external: dirs names 'egress' and / or 'ingress'")
            dmask |= bits[x]
        nd = bin(dmask).count("1")
        ids = np.ascontiguousarray(if_ids, np.uint32)
        a = np.asarray(addrs)
        v16 = a.ndim == 2
        a = np.ascontiguousarray(a, np.uint8).reshape(-1, 16) if v16 else np.ascontiguousarray(a, np.uint32)
        pr, sp = np.ascontiguousarray(protos, np.uint8), np.ascontiguousarray(sports, np.uint16)
        dp = np.ascontiguousarray(dports, np.uint16)
        n, p = len(ids), len(pr)
        if len(a) != n or len(sp) != p or len(dp) != p:
            raise ClsError("reach external: N interface ids and addresses, P protocols and ports")
        spec = _abi.ReachSpec(_abi.AF_V16 if v16 else _abi.AF_V4, n, _ptr(ids), None if v16 else _ptr(a),
                              _ptr(a) if v16 else None, p, _ptr(pr), _ptr(sp), _ptr(dp))
        k = np.zeros(1, np.uint32)
        fn = _abi.lib().cls_reach_external
        names = ("ranges", "total", "runs", "allow_addrs", "hist")
        if out is None:
            total = np.zeros(1, np.uint64)
            if cap is None:
                o = _abi.ReachExtOut(None, 0, _ptr(total), None, None, None, _ptr(k))
                self._check(fn(self.h, C.byref(spec), int(ext_if), dmask, C.byref(o), flags, None))
                cap = int(total[0])
            cap = int(cap)
            rec = np.zeros(cap, _abi.ADDR_RANGE) if cap > 0 else None
            runs, allow = np.zeros((nd, p, n), np.uint32), np.zeros((nd, p, n), np.uint64)
            hist = np.zeros((nd, p, 4), np.uint64)
            o = _abi.ReachExtOut(_ptr(rec), cap, _ptr(total), _ptr(runs), _ptr(allow), _ptr(hist), _ptr(k))
            self._check(fn(self.h, C.byref(spec), int(ext_if), dmask, C.byref(o), flags, None))
            if rec is not None:
                rec = rec[:min(int(total[0]), cap)]
            return dict(zip(names, (rec, int(total[0]), runs, allow, hist)), n_classes=int(k[0]))
        import torch
        res = list(out)
        if len(res) != 5:
            raise ClsError("reach external: out is (ranges, total, runs, allow_addrs, hist)")
        if cap is None:
            if res[0] is None:
                raise ClsError("reach external: the device form needs cap or a ranges tensor")
            cap = res[0].shape[0]
        cap = int(cap)
        shapes = ((cap, 4), (1,), (nd, p, n), (nd, p, n), (nd, p, 4))
        kinds = ((torch.int32, 4), (torch.int64, 8), (torch.int32, 4), (torch.int64, 8), (torch.int64, 8))
        for i, (sh, (dt, sz)) in enumerate(zip(shapes, kinds)):
            if i == 0 and cap == 0:
                res[0] = None
            elif res[i] is None:
                res[i] = torch.empty(sh, dtype=dt, device="cuda")
            elif not (_is_torch(res[i]) and res[i].is_cuda and res[i].is_contiguous() and
                      res[i].element_size() == sz and tuple(res[i].shape) == sh):
                raise ClsError("reach external: out[%d] must be a contiguous GPU tensor of shape %s, %d-byte "
                               "elements" % (i, sh, sz))
        s = None
        if stream is not None:
            s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        o = _abi.ReachExtOut(_ptr(res[0]), cap, _ptr(res[1]), _ptr(res[2]), _ptr(res[3]), _ptr(res[4]), _ptr(k))
        self._check(fn(self.h, C.byref(spec), int(ext_if), dmask, C.byref(o), flags | _abi.F_DEVICE, s))
        return dict(zip(names, res), n_classes=int(k[0]))

    def reach_hops(self, if_ids, addrs, protos, sports, dports, max_hops: int = 0, matrix=None, mode: str = "auto",
                   count: bool = False, hops: bool = True, reach: bool = True, exposed: bool = True,
                   levels: bool = True, closure: bool = False, out=None, stream=None):
        """The multi-hop closure of the reachability matrix (cls_reach_hops):
        endpoint s has an edge to d != s when some probe's cell (p, s, d) is
        CONN_ALLOW.  Returns ReachHops(hops [N, N] u8: the length of a
        shortest path s -> d if at most ``max_hops`` (0: 254), else 255, and 0
        on the diagonal; reach [N] u32: the destinations a source reaches;
        exposed [N] u32: the sources that reach a destination; levels [256]
        u64: pairs per hops value; closure [N, (N + 63) // 64] u64: bit d of
        row s set when s reaches d or s == d); what is not wanted is None.
        ``matrix`` None: the matrix of reach_matrix's arguments is evaluated on
        the device (mode and count as there) and never stored.  ``matrix`` a
        [P, N, N] uint8 array of an earlier call: it is folded instead, nothing
        is evaluated, and if_ids, addrs and the probe arrays may be None.  out
        None: numpy results (the call returns with them), for a numpy matrix
        or none.  out a sequence (hops, reach, exposed, levels, closure) of
        contiguous torch GPU tensors -- u8, 4-, 4-, 8-, 8-byte elements; None
        for a wanted one allocates it -- selects the device form, which a
        torch GPU matrix requires: the call only enqueues on ``stream``
        (default: the engine's) and returns the tensors."""
        flags = {"auto": 0, "classifier": _abi.F_CONN_CLS, "linear": _abi.F_FORCE_LINEAR}[mode]
        if count:
            flags |= _abi.F_COUNT
        if matrix is None:
            ids = np.ascontiguousarray(if_ids, np.uint32)
            a = np.asarray(addrs)
            v16 = a.ndim == 2
            a = np.ascontiguousarray(a, np.uint8).reshape(-1, 16) if v16 else np.ascontiguousarray(a, np.uint32)
            pr, sp = np.ascontiguousarray(protos, np.uint8), np.ascontiguousarray(sports, np.uint16)
            dp = np.ascontiguousarray(dports, np.uint16)
            n, p = len(ids), len(pr)
            if len(a) != n or len(sp) != p or len(dp) != p:
                raise ClsError("reach hops: N interface ids and addresses, P protocols and ports")
            spec = _abi.ReachSpec(_abi.AF_V16 if v16 else _abi.AF_V4, n, _ptr(ids), None if v16 else _ptr(a),
                                  _ptr(a) if v16 else None, p, _ptr(pr), _ptr(sp), _ptr(dp))
        else:
            if _is_torch(matrix):
                import torch
                if out is None:
                    raise ClsError("reach hops: a GPU matrix needs the device form (out)")
                ok = matrix.is_cuda and matrix.is_contiguous() and matrix.dtype == torch.uint8
            else:
                if out is not None:
                    raise ClsError("reach hops: the device form takes a GPU matrix")
                matrix = np.asarray(matrix)
                ok = matrix.dtype == np.uint8 and matrix.flags.c_contiguous
            if not ok or matrix.ndim != 3 or matrix.shape[1] != matrix.shape[2]:
                raise ClsError("reach hops: matrix must be a contiguous uint8 array of shape (P, N, N)")
            p, n = int(matrix.shape[0]), int(matrix.shape[1])
            spec = _abi.ReachSpec(_abi.AF_V4, n, None, None, None, p, None, None, None)
        w = (n + 63) // 64
        want = (hops, reach, exposed, levels, closure)
        shapes = ((n, n), (n,), (n,), (256,), (n, w))
        if out is None:
            res = [np.zeros(sh, dt) if wt else None
                   for wt, sh, dt in zip(want, shapes, (np.uint8, np.uint32, np.uint32, np.uint64, np.uint64))]
            s = None
        else:
            import torch
            flags |= _abi.F_DEVICE
            res = list(out)
            if len(res) != 5:
                raise ClsError("reach hops: out is (hops, reach, exposed, levels, closure)")
            kinds = ((torch.uint8, 1), (torch.int32, 4), (torch.int32, 4), (torch.int64, 8), (torch.int64, 8))
            for k, (wt, sh, (dt, sz)) in enumerate(zip(want, shapes, kinds)):
                if not wt:
                    res[k] = None
                elif res[k] is None:
                    res[k] = torch.empty(sh, dtype=dt, device="cuda")
                elif not (_is_torch(res[k]) and res[k].is_cuda and res[k].is_contiguous() and
                          res[k].element_size() == sz and tuple(res[k].shape) == sh):
                    raise ClsError("reach hops: out[%d] must be a contiguous GPU tensor of shape %s, %d-byte "
                                   "elements" % (k, sh, sz))
            s = None
            if stream is not None:
                s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream
        o = _abi.ReachHopsOut(*[_ptr(x) for x in res])
        self._check(_abi.lib().cls_reach_hops(self.h, C.byref(spec), _ptr(matrix), int(max_hops), C.byref(o), flags, s))
        return ReachHops(*res)

    def reach_classes(self, if_ids, addrs, protos, sports, dports, matrix=None, mode: str = "auto",
                      device: bool = False, verdict: bool = False, class_cap: int = 64, stream=None):
        """The endpoints the reachability matrix cannot tell apart, and the
        matrix between their classes (cls_reach_classes): s and t are in one
        class iff exchanging them leaves the [P, N, N] matrix unchanged.
        Returns ReachClasses(classes [N] u32, numbered by ascending smallest
        member; reps [C] u32, each class's smallest member; sizes [C] u32;
        self_ [P, C] u8, a class's diagonal value; quotient [P, C, C] u8, the
        value between classes, on its diagonal the value between two members
        of a class, 255 for a one-member class; rounds, 1 unless the
        classes_key_bits option forces collisions; verdict, the [P, N, N]
        matrix when ``verdict``, else None).  expand_classes(classes, self_,
        quotient) is the matrix again.  ``matrix`` None: the matrix of
        reach_matrix's arguments is evaluated on the device (mode as there).
        ``matrix`` a [P, N, N] uint8 array of an earlier call: it is summarised
        instead, and the other arrays may be None.  ``device``: the results
        (and a given matrix) are torch GPU tensors, the work runs on
        ``stream`` (default: the engine's); either way the call returns with
        the results complete.  ``class_cap``: the classes the first call has
        room for; with more, the call is made once more with room for all."""
        flags = {"auto": 0, "classifier": _abi.F_CONN_CLS, "linear": _abi.F_FORCE_LINEAR}[mode]
        if matrix is None:
            ids = np.ascontiguousarray(if_ids, np.uint32)
            a = np.asarray(addrs)
            v16 = a.ndim == 2
            a = np.ascontiguousarray(a, np.uint8).reshape(-1, 16) if v16 else np.ascontiguousarray(a, np.uint32)
            pr, sp = np.ascontiguousarray(protos, np.uint8), np.ascontiguousarray(sports, np.uint16)
            dp = np.ascontiguousarray(dports, np.uint16)
            n, p = len(ids), len(pr)
            if len(a) != n or len(sp) != p or len(dp) != p:
                raise ClsError("reach classes: N interface ids and addresses, P protocols and ports")
            spec = _abi.ReachSpec(_abi.AF_V16 if v16 else _abi.AF_V4, n, _ptr(ids), None if v16 else _ptr(a),
                                  _ptr(a) if v16 else None, p, _ptr(pr), _ptr(sp), _ptr(dp))
        else:
            if _is_torch(matrix):
                import torch
                if not device:
                    raise ClsError("reach classes: a GPU matrix needs the device form (device=True)")
                ok = matrix.is_cuda and matrix.is_contiguous() and matrix.dtype == torch.uint8
            else:
                if device:
                    raise ClsError("reach classes: the device form takes a GPU matrix")
                matrix = np.asarray(matrix)
                ok = matrix.dtype == np.uint8 and matrix.flags.c_contiguous
            if not ok or matrix.ndim != 3 or matrix.shape[1] != matrix.shape[2]:
                raise ClsError("reach classes: matrix must be a contiguous uint8 array of shape (P, N, N)")
            p, n = int(matrix.shape[0]), int(matrix.shape[1])
            spec = _abi.ReachSpec(_abi.AF_V4, n, None, None, None, p, None, None, None)
        s = None
        if device:
            import torch
            flags |= _abi.F_DEVICE
            if stream is not None:
                s = stream.cuda_stream if hasattr(stream, "cuda_stream") else stream

            def new(shape, size):
                return torch.empty(shape, dtype={1: torch.uint8, 4: torch.int32}[size], device="cuda")
        else:
            def new(shape, size):
                return np.zeros(shape, {1: np.uint8, 4: np.uint32}[size])
        classes = new((n,), 4)
        v = new((p, n, n), 1) if verdict else None
        c, rounds = np.zeros(1, np.uint32), np.zeros(1, np.uint32)
        cap = max(1, int(class_cap))
        for _ in range(2):
            reps, sizes, self_, quot = new((cap,), 4), new((cap,), 4), new((p, cap), 1), new((p, cap, cap), 1)
            o = _abi.ReachClassesOut(_ptr(classes), _ptr(c), cap, _ptr(reps), _ptr(sizes), _ptr(self_), _ptr(quot),
                                     _ptr(v), _ptr(rounds), None)
            self._check(_abi.lib().cls_reach_classes(self.h, C.byref(spec), _ptr(matrix), C.byref(o), flags, s))
            if int(c[0]) <= cap:
                break
            cap = int(c[0])                              # (the per-class outputs were left alone)
        k = int(c[0])
        if k != cap:
            # the C ABI's arrays are dense in C: the first C classes of each
            reps, sizes = reps[:k], sizes[:k]
            self_ = self_.reshape(-1)[:p * k].reshape(p, k)
            quot = quot.reshape(-1)[:p * k * k].reshape(p, k, k)
        return ReachClasses(classes, reps, sizes, self_, quot, int(rounds[0]), v)

    def stream_floor_conn(self, src_if, dst_if, src, dst, proto, sport, dport, reps: int = 20) -> float:
        """The connection path's HBM floor on a device batch (cls_stream_floor_conn):
        ms per launch of a kernel that reads the same 22 B per IPv4 connection
        and writes one byte, with no evaluation."""
        import torch
        n = src.shape[0]
        out = torch.empty(n, dtype=torch.uint8, device=src.device)
        pk = _abi.PktSoa(_abi.AF_V4, _ptr(src), _ptr(dst), None, None, _ptr(sport), _ptr(dport), _ptr(proto))
        cs = _abi.ConnSoa(pk, _ptr(src_if), _ptr(dst_if))
        ms = C.c_float()
        self._check(_abi.lib().cls_stream_floor_conn(self.h, C.byref(cs), n, _ptr(out), reps, C.byref(ms), None))
        return ms.value

    def conn_counters(self, table, reset: bool = False) -> np.ndarray:
        """Per-rule connection counters of a table (a Table, a table id or an
        installed ACL's name): R + 1 u64, [R] = default DENY."""
        if isinstance(table, str):
            table = self.acl_table(table)
        tid = table.id if isinstance(table, Table) else int(table)
        info = _abi.TableInfo()
        self._check(_abi.lib().cls_table_get_info(self.h, tid, C.byref(info)))
        out = np.zeros(info.n_rules + 1, np.uint64)
        self._check(_abi.lib().cls_conn_counters(self.h, tid, _ptr(out), 1 if reset else 0))
        return out


_BF_BYTES = {_abi.BF_SPORT: 2, _abi.BF_DPORT: 2, _abi.BF_PROTO: 1, _abi.BF_VERDICT: 1,
             _abi.BF_SRC_IF: 4, _abi.BF_DST_IF: 4}
_NP = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def shard_range(n: int, n_shards: int, shard: int):
    """(first, count) of shard ``shard`` of n packets (cls_shard_range)."""
    a, b = C.c_uint64(0), C.c_uint64(0)
    rc = _abi.lib().cls_shard_range(n, n_shards, shard, C.byref(a), C.byref(b))
    if rc != 0:
        raise ClsError("cls_shard_range(%d, %d, %d): rc=%d" % (n, n_shards, shard, rc))
    return a.value, b.value


class Batch:
    """An engine-owned packet (or connection) batch in HBM, sharded over the
    engine's devices (cls_batch_*): no torch, no caller pointer kept."""

    def __init__(self, engine: Engine, n: int, af: int = _abi.AF_V4, conn: bool = False, mirror: bool = False):
        self.engine, self.n, self.af = engine, n, af
        flags = (_abi.BATCH_CONN if conn else 0) | (_abi.BATCH_MIRROR if mirror else 0)
        h = C.c_void_p()
        engine._check(_abi.lib().cls_batch_create(engine.h, af, n, flags, C.byref(h)))
        self.h = h
        engine._batches.add(self)

    def close(self):
        if getattr(self, "h", None):
            _abi.lib().cls_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _elem(self, field: int) -> int:
        return _BF_BYTES.get(field, 16 if self.af == _abi.AF_V16 else 4)

    def shards(self):
        """[(device, first, n)] per shard."""
        k = C.c_uint32(0)
        self.engine._check(_abi.lib().cls_batch_shards(self.h, C.byref(k)))
        out = []
        for g in range(k.value):
            d, a, b = C.c_int(0), C.c_uint64(0), C.c_uint64(0)
            self.engine._check(_abi.lib().cls_batch_shard(self.h, g, C.byref(d), C.byref(a), C.byref(b)))
            out.append((d.value, a.value, b.value))
        return out

    def field_ptr(self, shard: int, field: int) -> int:
        p = C.c_void_p()
        self.engine._check(_abi.lib().cls_batch_field(self.h, shard, field, C.byref(p)))
        return p.value

    def mirror(self, field: int) -> np.ndarray:
        """The pinned host mirror of a field (CLS_BATCH_MIRROR) as a numpy view."""
        p = C.c_void_p()
        self.engine._check(_abi.lib().cls_batch_mirror(self.h, field, C.byref(p)))
        eb = self._elem(field)
        buf = (C.c_uint8 * (self.n * eb)).from_address(p.value)
        a = np.frombuffer(buf, np.uint8)
        return a.reshape(-1, 16) if eb == 16 else a.view(_NP[eb])

    def upload(self, field: int, arr=None, first: int = 0, n: Optional[int] = None):
        """Packets [first, first+n) of a field from ``arr`` (None: the mirror)."""
        eb = self._elem(field)
        if arr is not None:
            arr = np.ascontiguousarray(arr, np.uint8 if eb == 16 else _NP[eb])
            n = len(arr) if n is None else n
        n = (self.n - first) if n is None else n
        self.engine._check(_abi.lib().cls_batch_upload(self.h, field, first, n, _ptr(arr)))

    def download(self, field: int, first: int = 0, n: Optional[int] = None, mirror: bool = False):
        n = (self.n - first) if n is None else n
        eb = self._elem(field)
        if mirror:
            self.engine._check(_abi.lib().cls_batch_download(self.h, field, first, n, None))
            return None
        out = np.zeros((n, 16) if eb == 16 else n, np.uint8 if eb == 16 else _NP[eb])
        self.engine._check(_abi.lib().cls_batch_download(self.h, field, first, n, _ptr(out)))
        return out

    def gen_traffic(self, spec: dict, stream_first: int = 0):
        """The synthetic stream generated on the devices: batch packet i =
        stream packet stream_first + i."""
        if self.af == _abi.AF_V16:
            ts, keep = _spec16(spec)
            self.engine._check(_abi.lib().cls_batch_gen_traffic_v16(self.h, C.byref(ts), stream_first))
        else:
            ts, keep = _spec4(spec)
            self.engine._check(_abi.lib().cls_batch_gen_traffic_v4(self.h, C.byref(ts), stream_first))
        del keep

    def counters(self, n_rules: int) -> np.ndarray:
        out = np.zeros(n_rules + 1, np.uint64)
        self.engine._check(_abi.lib().cls_batch_counters(self.h, _ptr(out), n_rules + 1))
        return out

    def wait(self):
        self.engine._check(_abi.lib().cls_batch_wait(self.h))


def _spec4(spec: dict):
    pods = np.ascontiguousarray(spec.get("pod_ips", []), np.uint32)
    da = np.ascontiguousarray(spec.get("dst_addrs", []), np.uint32)
    dl = np.ascontiguousarray(spec.get("dst_lens", []), np.uint8)
    ports = np.ascontiguousarray(spec.get("ports", []), np.uint16)
    ts = _abi.TrafficSpec(spec["seed"], spec.get("pct_pod_src", 60), spec.get("pct_rule_dst", 50),
                          spec.get("pct_table_port", 50), spec.get("pct_icmp", 0),
                          pods.ctypes.data, len(pods), da.ctypes.data, dl.ctypes.data, len(da),
                          ports.ctypes.data, len(ports))
    return ts, (pods, da, dl, ports)


def _spec16(spec: dict):
    pods = np.ascontiguousarray(spec.get("pod_ips", np.zeros((0, 16))), np.uint8)
    da = np.ascontiguousarray(spec.get("dst_addrs", np.zeros((0, 16))), np.uint8)
    dl = np.ascontiguousarray(spec.get("dst_lens", []), np.uint8)
    ports = np.ascontiguousarray(spec.get("ports", []), np.uint16)
    ts = _abi.TrafficSpec16(spec["seed"], spec.get("pct_pod_src", 60), spec.get("pct_rule_dst", 50),
                            spec.get("pct_table_port", 50), spec.get("pct_icmp", 0),
                            pods.ctypes.data, len(pods), da.ctypes.data, dl.ctypes.data, len(da),
                            ports.ctypes.data, len(ports))
    return ts, (pods, da, dl, ports)


def _ip16(ip: Optional[bytes]) -> Optional[bytes]:
    """net.IP as the 16-byte form (IPv4 as IPv4-mapped, like Go's To16)."""
    if ip is None or len(ip) not in (4, 16):
        return None
    return bytes(10) + b"\xff\xff" + bytes(ip) if len(ip) == 4 else bytes(ip)


def _ip4(ip: Optional[bytes]) -> Optional[int]:
    if ip is None:
        return None
    x = gonet.to4(ip)
    if x is None:
        return None
    return int.from_bytes(x, "big")


def v6_rules(rules):
    """The indices of the rules with an IPv6 (family-16) source or
    destination network: an IPv4 sweep sees them as dead, and they exist for
    packets it does not cover."""
    out = []
    for k, r in enumerate(rules):
        ipr = r.matches.ip_rule if r.matches is not None else None
        ip = ipr.ip if ipr is not None else None
        if ip is None:
            continue
        for s in (ip.source_network, ip.destination_network):
            net = gonet.parse_cidr(s)[1] if s else None
            nn = net._network_number_and_mask()[0] if net is not None else None
            if nn is not None and len(nn) == 16:
                out.append(k)
                break
    return out


def minimize_rounds(sweep, n_rules: int, keep=(), max_rounds: int = 64):
    """The round loop of ACLEngine.acl_minimize over any form of the sweep:
    ``sweep(skip)`` returns table_need's dict for the set ``skip`` of deleted
    rules.  Each round deletes every free rule outside ``keep`` -- all free
    rules can go together without changing a verdict, and while a rule is dead
    or redundant at least one is free (the highest redundant rule can only
    fall to rules above it, none of them redundant) --; it stops when no rule
    outside ``keep`` is dead or redundant, or after ``max_rounds``.  Returns
    (kept rule indices, removed indices per round)."""
    keep = set(int(k) for k in keep)
    skip, rounds = set(), []
    for _ in range(max_rounds):
        r = sweep(sorted(skip))
        loose = [k for k in range(n_rules) if k not in keep and k not in skip and
                 r["need"][k] in (_abi.NEED_DEAD, _abi.NEED_REDUNDANT)]
        if not loose:
            break
        gone = [k for k in loose if r["free"][k]]
        if not gone:              # only where keep pins the rules the loose ones fall to
            break
        rounds.append(gone)
        skip.update(gone)
    return [k for k in range(n_rules) if k not in skip], rounds


class ACLEngine:
    """MockACLEngine drop-in over the GPU engine (aclengine_mock.go:94-471)."""

    def __init__(self, contiv, engine: Optional[Engine] = None):
        self.contiv = contiv
        self.engine = engine or Engine()
        self.pods = {}              # PodID -> (net.IP bytes | None, another_node)
        self.by_name = {}           # ACL name -> Acl (the protobuf the host keeps)

    # RegisterPod (:144-148)
    def register_pod(self, pod, pod_ip: str, another_node: bool):
        self.pods[pod] = (gonet.parse_ip(pod_ip), another_node)

    # ApplyTxn (:151-198): returns an error string or None
    def apply_txn(self, ops):
        for key, value in ops:
            if not key.startswith(ACL_KEY_PREFIX):
                return "non-ACL changed in txn"
            name = key[len(ACL_KEY_PREFIX):]
            if value is not None:
                acl = value.clone()          # the engine keeps its own message (rules shared, never modified)
                ifs = acl.interfaces
                rc = self.engine.acl_put(acl.acl_name, acl.rules,
                                         ifs.ingress if ifs else [], ifs.egress if ifs else [])
                if rc != 0:
                    return _abi.lib().cls_last_error(self.engine.h).decode()
                self.by_name[acl.acl_name] = acl
            else:
                rc = self.engine.acl_del(name)
                if rc != 0:
                    return _abi.lib().cls_last_error(self.engine.h).decode()
                self.by_name.pop(name, None)
        return None

    def dump_acls(self):
        return list(self.by_name.values())

    def get_num_of_acls(self) -> int:
        return self.engine.acl_counts()[0]

    def get_num_of_acl_changes(self) -> int:
        return self.engine.acl_counts()[1]

    def _acl_of_table(self, tid: int):
        """The protobuf ACL whose compiled table the engine bound (-1: nil)."""
        if tid < 0:
            return None
        for name, acl in self.by_name.items():
            if self.engine.acl_table(name) == tid:
                return acl
        return None

    def get_inbound_acl(self, if_name: str):
        i, _ = self.engine.if_acls(self.engine.if_id(if_name))
        return self._acl_of_table(i)

    def get_outbound_acl(self, if_name: str):
        _, o = self.engine.if_acls(self.engine.if_id(if_name))
        return self._acl_of_table(o)

    def get_acl_by_name(self, name: str):
        return self.by_name.get(name)

    # -- Connection* (:243-390), resolved on the host, evaluated on the GPU --
    def _node_output_if(self):
        ifn = self.contiv.get_vxlan_bvi_if_name()
        return ifn if ifn != "" else self.contiv.get_main_physical_if_name()

    def _pod_if(self, pod, cfg):
        if cfg[1]:
            ifn = self._node_output_if()
            return ifn if ifn != "" else None
        ifn, ok = self.contiv.get_if_name(pod.namespace, pod.name)
        return ifn if ok else None

    def resolve(self, fn: str, args):
        """Returns (src_if, src_ip, dst_if, dst_ip, proto, sport, dport) or
        CONN_FAILURE when the reference fails before testConnection."""
        if fn == "ConnectionPodToPod":
            sp, dp, proto, sport, dport = args
            s, d = self.pods.get(sp), self.pods.get(dp)
            if s is None or d is None:
                return CONN_FAILURE
            sif, dif = self._pod_if(sp, s), self._pod_if(dp, d)
            if sif is None or dif is None:
                return CONN_FAILURE
            return sif, s[0], dif, d[0], proto, sport, dport
        if fn == "ConnectionPodToInternet":
            sp, dst_ip, proto, sport, dport = args
            s = self.pods.get(sp)
            if s is None or s[1]:
                return CONN_FAILURE
            sif, ok = self.contiv.get_if_name(sp.namespace, sp.name)
            dif = self._node_output_if()
            ip = gonet.parse_ip(dst_ip)
            if not ok or dif == "" or ip is None:
                return CONN_FAILURE
            return sif, s[0], dif, ip, proto, sport, dport
        src_ip, dp, proto, sport, dport = args
        d = self.pods.get(dp)
        if d is None or d[1]:
            return CONN_FAILURE
        sif = self._node_output_if()
        ip = gonet.parse_ip(src_ip)
        dif, ok = self.contiv.get_if_name(dp.namespace, dp.name)
        if sif == "" or ip is None or not ok:
            return CONN_FAILURE
        return sif, ip, dif, d[0], proto, sport, dport

    def connection_batch(self, calls, count: bool = False):
        """calls: list of (fn name, args).  One GPU launch for all of them: the
        IPv4 layout when every endpoint is IPv4, else the 16-byte layout."""
        return self._connections(calls, count, False)

    def connection_trace(self, calls):
        """connection_batch with the matched rules the reference logs
        (aclengine_mock.go:651-654): per call (ConnectionAction, [(ACL name,
        rule index or None for the default DENY) of every evalACL call
        testConnection made on a non-nil ACL, in its order]) -- a call that
        fails before testConnection has an empty list.  One GPU launch
        (Engine.connect_rules); no counters."""
        return self._connections(calls, False, True)

    def _connections(self, calls, count: bool, trace: bool):
        # (a call the reference fails before testConnection stays a Failure)
        out = [(CONN_FAILURE, []) if trace else CONN_FAILURE for _ in calls]
        rows = []
        for i, (fn, args) in enumerate(calls):
            r = self.resolve(fn, args)
            if r == CONN_FAILURE:
                continue
            sif, sip, dif, dip, proto, sport, dport = r
            rows.append((i, self.engine.if_id(sif), self.engine.if_id(dif), sip, dip, proto, sport, dport))
        if not rows:
            return out
        four = [(_ip4(r[3]), _ip4(r[4])) for r in rows]
        meta = np.array([(r[1], r[2], r[5], r[6], r[7]) for r in rows], np.int64)
        if all(a is not None and b is not None for a, b in four):
            src = np.array([a for a, _ in four], np.uint32)
            dst = np.array([b for _, b in four], np.uint32)
        else:
            a16 = [(_ip16(r[3]), _ip16(r[4])) for r in rows]
            if any(a is None or b is None for a, b in a16):
                raise ClsError("connection endpoint is not an IPv4 or IPv6 address")
            src = np.frombuffer(b"".join(a for a, _ in a16), np.uint8).reshape(-1, 16)
            dst = np.frombuffer(b"".join(b for _, b in a16), np.uint8).reshape(-1, 16)
        if trace:
            res, rules = self.engine.connect_rules(meta[:, 0], meta[:, 1], src, dst, meta[:, 2], meta[:, 3],
                                                   meta[:, 4])
            names = {}                              # table id -> (ACL name, R)

            def acl(tid):
                if tid not in names:
                    a = self._acl_of_table(tid)
                    names[tid] = (a.acl_name, len(a.rules))
                return names[tid]
            for (i, s_id, d_id, *_), v, row in zip(rows, res, rules):
                (s_in, s_out), (d_in, d_out) = self.engine.if_acls(s_id), self.engine.if_acls(d_id)
                made = []
                for tid, rule in zip((s_in, d_out, d_in, s_out), row):
                    if rule >= 0:
                        name, n_rules = acl(tid)
                        made.append((name, int(rule) if rule < n_rules else None))
                out[i] = (int(v), made)
            return out
        res = self.engine.connect_batch(meta[:, 0], meta[:, 1], src, dst, meta[:, 2], meta[:, 3], meta[:, 4],
                                        count=count)
        for (i, *_), v in zip(rows, res):
            out[i] = int(v)
        return out

    def _matrix_endpoints(self, pods):
        """(index in pods, interface id, net.IP) of the pods that reach
        testConnection (connection_matrix)."""
        eps = []
        for i, pod in enumerate(pods):
            cfg = self.pods.get(pod)
            ifn = self._pod_if(pod, cfg) if cfg is not None else None
            if ifn is not None:
                eps.append((i, self.engine.if_id(ifn), cfg[0]))
        return eps

    @staticmethod
    def _matrix_addrs(eps):
        """The endpoints' addresses: u32 when all are IPv4, else (n, 16) bytes."""
        four = [_ip4(ip) for _, _, ip in eps]
        if all(a is not None for a in four):
            return np.array(four, np.uint32)
        a16 = [_ip16(ip) for _, _, ip in eps]
        if any(a is None for a in a16):
            raise ClsError("connection endpoint is not an IPv4 or IPv6 address")
        return np.frombuffer(b"".join(a16), np.uint8).reshape(-1, 16)

    def connection_matrix(self, pods, probes, count: bool = False) -> np.ndarray:
        """Who reaches whom: a [len(probes), len(pods), len(pods)] uint8 array
        whose cell (p, s, d) equals connection_pod_to_pod(pods[s], pods[d],
        *probes[p]) (ConnectionPodToPod, :243-300), probes being (proto,
        sport, dport) triples -- one engine call (Engine.reach_matrix) over
        the pods' endpoints instead of a row per cell.  Pods the reference
        fails before testConnection (unregistered, no interface, no node
        output interface) stay out of the engine call: their rows and columns
        are CONN_FAILURE.  The IPv4 layout when every endpoint is IPv4, else
        the 16-byte layout.  count: as connection_batch."""
        out = np.full((len(probes), len(pods), len(pods)), CONN_FAILURE, np.uint8)
        eps = self._matrix_endpoints(pods)
        if not eps or not probes:
            return out
        addrs = self._matrix_addrs(eps)
        pr = np.array(probes, np.int64).reshape(-1, 3)
        v, _, _ = self.engine.reach_matrix([e[1] for e in eps], addrs, pr[:, 0], pr[:, 1], pr[:, 2], count=count,
                                           hist=False, allow=False)
        at = np.array([e[0] for e in eps])
        out[:, at[:, None], at[None, :]] = v
        return out

    def connection_hops(self, pods, probes, max_hops: int = 0) -> np.ndarray:
        """Lateral movement: a [len(pods), len(pods)] uint8 array whose cell
        (s, d) is the least number of connections, each CONN_ALLOW under some
        probe of ``probes`` ((proto, sport, dport) triples), that lead from
        pods[s] to pods[d] through other pods of ``pods`` -- 0 for s == d, 255
        when there is no such path of at most ``max_hops`` (0: 254)
        connections.  One engine call (Engine.reach_hops) over the pods'
        endpoints; the matrix is never brought to the host.  A pod the
        reference fails before testConnection (connection_matrix) has no
        edges: its row and column are 255 but for the diagonal."""
        n = len(pods)
        out = np.full((n, n), _abi.HOPS_NONE, np.uint8)
        out[np.arange(n), np.arange(n)] = 0
        eps = self._matrix_endpoints(pods)
        if not eps or not probes:
            return out
        pr = np.array(probes, np.int64).reshape(-1, 3)
        r = self.engine.reach_hops([e[1] for e in eps], self._matrix_addrs(eps), pr[:, 0], pr[:, 1], pr[:, 2],
                                   max_hops=max_hops, reach=False, exposed=False, levels=False)
        at = np.array([e[0] for e in eps])
        out[at[:, None], at[None, :]] = r.hops
        return out

    def connection_classes(self, pods, probes):
        """The connectivity map of ``pods`` under ``probes`` ((proto, sport,
        dport) triples): (groups, self_, quotient).  groups: lists of pod ids,
        the pods that connection_matrix(pods, probes) cannot tell apart --
        exchanging two pods of a group leaves it unchanged -- ordered by their
        first pod in ``pods``; self_ [P, C]: a group's pods to themselves;
        quotient [P, C, C]: the ConnectionAction from any pod of group a to
        any of group b, on the diagonal between two pods of one group (255 for
        a group of one).  One engine call (Engine.reach_classes) over the
        pods' endpoints; with pods the reference fails before testConnection
        (rows and columns of CONN_FAILURE) the matrix is evaluated first and
        summarised whole."""
        n_p = len(probes)
        if not pods:
            return [], np.zeros((n_p, 0), np.uint8), np.zeros((n_p, 0, 0), np.uint8)
        if not probes:                                   # nothing tells the pods apart
            return [list(pods)], np.zeros((0, 1), np.uint8), np.zeros((0, 1, 1), np.uint8)
        eps = self._matrix_endpoints(pods)
        if len(eps) == len(pods):
            pr = np.array(probes, np.int64).reshape(-1, 3)
            r = self.engine.reach_classes([e[1] for e in eps], self._matrix_addrs(eps), pr[:, 0], pr[:, 1], pr[:, 2])
        else:
            r = self.engine.reach_classes(None, None, None, None, None, matrix=self.connection_matrix(pods, probes))
        groups = [[] for _ in range(len(r.reps))]
        for pod, c in zip(pods, r.classes.tolist()):
            groups[c].append(pod)
        return groups, r.self_, r.quotient

    def connection_ports(self, pods, protocol, src_port):
        """On which destination ports pod s reaches pod d: (ranges, runs),
        ranges the maximal (src, dst, port_lo, port_hi, action) tuples -- src
        and dst indices into ``pods`` -- in (src, dst, port_lo) order, such
        that connection_pod_to_pod(pods[src], pods[dst], protocol, src_port,
        port) == action for every port of the range, and runs the
        [len(pods), len(pods)] number of ranges per pair.  One engine call
        (Engine.reach_ports) over the resolvable endpoints; the pairs of a
        pod the reference fails before testConnection (connection_matrix) are
        the one range 0..65535 of CONN_FAILURE."""
        n = len(pods)
        runs = np.ones((n, n), np.uint32)
        eps = self._matrix_endpoints(pods)
        per = {}                                    # (src, dst) -> its ranges
        if eps:
            r = self.engine.reach_ports([e[1] for e in eps], self._matrix_addrs(eps), protocol, src_port)
            at = np.array([e[0] for e in eps])
            runs[at[:, None], at[None, :]] = r.runs
            for c in r.ranges:
                per.setdefault((int(at[c["src"]]), int(at[c["dst"]])), []).append(
                    (int(c["port_lo"]), int(c["port_hi"]), int(c["action"])))
        ranges = []
        for s in range(n):
            for d in range(n):
                for lo, hi, act in per.get((s, d), [(0, 65535, CONN_FAILURE)]):
                    ranges.append((s, d, lo, hi, act))
        return ranges, runs

    def connection_external(self, pods, probes, dirs=("egress", "ingress")):
        """Which remote IPv4 addresses each pod reaches and which reach it: a
        dict (dir, probe index, pod index) -> the list of maximal (addr_lo,
        addr_hi, action) ranges, ascending and covering 0 .. 0xFFFFFFFF, such
        that connection_pod_to_internet(pods[s], a, *probes[p]) == action
        ("egress") or connection_internet_to_pod(a, pods[s], *probes[p]) ==
        action ("ingress") for every address a of the range
        (ConnectionPodToInternet :303-346, ConnectionInternetToPod :349-390),
        probes being (proto, sport, dport) triples and dir the name given in
        ``dirs``.  One engine call (Engine.reach_external) over the pods that
        reach testConnection; a pod the reference fails before it
        (unregistered, on another node, without an interface, or with an
        empty node output interface name) has the one range (0, 0xFFFFFFFF,
        CONN_FAILURE)."""
        dirs = [dirs] if isinstance(dirs, str) else list(dirs)
        for d in dirs:
            if d not in ("egress", "ingress"):
                raise ClsError("connection external: dirs names 'egress' and / or 'ingress'")
        out = {(d, p, s): [(0, 0xFFFFFFFF, CONN_FAILURE)]
               for d in dirs for p in range(len(probes)) for s in range(len(pods))}
        ext = self._node_output_if()
        eps = []
        for i, pod in enumerate(pods):
            cfg = self.pods.get(pod)
            if cfg is None or cfg[1] or ext == "":
                continue
            ifn, ok = self.contiv.get_if_name(pod.namespace, pod.name)
            if ok:
                eps.append((i, self.engine.if_id(ifn), cfg[0]))
        if not eps or not probes or not dirs:
            return out
        pr = np.array(probes, np.int64).reshape(-1, 3)
        order = [d for d in ("egress", "ingress") if d in dirs]
        r = self.engine.reach_external([e[1] for e in eps], self._matrix_addrs(eps), pr[:, 0], pr[:, 1], pr[:, 2],
                                       self.engine.if_id(ext), dirs=order)
        for e in eps:
            for d in dirs:
                for p in range(len(probes)):
                    out[(d, p, e[0])] = []
        for c in r["ranges"]:
            out[(("egress", "ingress")[c["dir"]], int(c["probe"]), eps[c["src"]][0])].append(
                (int(c["addr_lo"]), int(c["addr_hi"]), int(c["action"])))
        return out

    def acl_coverage(self, acl_name: str, af: int = 4):
        """Which rules of an installed ACL can never be the matched rule, and a
        packet for each of the others (Engine.table_cover over the ACL's
        compiled table; the reference has no such call -- the closest is the
        matched rule evalACL logs at Debug).  Returns a dict: ``dead``, the
        indices of the rules no packet terminates at; ``witness``, rule index
        -> (src string, dst string, protocol, dport), the least packet in
        (src, dst, protocol, dport) order that terminates at the rule,
        protocol 3 standing for every value above 2; ``default_reachable``,
        whether some packet falls through to the default DENY.  The sweep
        covers the IPv4 packet space only (``af`` 16: the same packets in the
        16-byte layout): a rule that only native IPv6 packets can reach is
        reported dead.  Raises ClsError for an unknown name."""
        tid = self.engine.acl_table(acl_name)
        if acl_name not in self.by_name or tid < 0:
            raise ClsError("acl coverage: no ACL %r" % (acl_name,))
        r = self.engine.table_cover(tid, af=af)
        n = len(r["live"]) - 1

        def ip(a):
            return "%d.%d.%d.%d" % (a >> 24, a >> 16 & 255, a >> 8 & 255, a & 255)
        wit = {k: (ip(int(w["src"])), ip(int(w["dst"])), int(w["proto"]), int(w["dport"]))
               for k, w in enumerate(r["witness"][:n]) if w["live"]}
        return {"dead": [k for k in range(n) if not r["live"][k]], "witness": wit,
                "default_reachable": bool(r["live"][n])}

    def acl_diff(self, acl_name: str, other, af: int = 4):
        """Whether an installed ACL and ``other`` -- another installed ACL's
        name, or a rule list such as a candidate replacement -- give every
        IPv4 packet the same ACLAction, and where they do not
        (Engine.table_diff; the reference has no such call).  A rule list is
        put as a temporary table and deleted again, also on error.  Returns a
        dict: ``equal``; ``n_diff`` and ``n_cells``, cells of the joint class
        product; ``pairs``, the 4 x 4 cells per (was, now) as lists;
        ``records``, the differing packets as (src_lo, src_hi, dst_lo,
        dst_hi) dotted quads, protocol (3 standing for every value above 2),
        port_lo, port_hi, was, now, rule_a, rule_b, ascending; ``rules_a``
        and ``rules_b``, rule index (the rule count: the default DENY) ->
        (differing cells, (src, dst, protocol, dport) of the least differing
        packet terminating there) for the rules responsible on either side.
        As acl_coverage, the diff covers the IPv4 packet space only.  Raises
        ClsError for an unknown name."""
        tid = self.engine.acl_table(acl_name)
        if acl_name not in self.by_name or tid < 0:
            raise ClsError("acl diff: no ACL %r" % (acl_name,))
        tmp = None
        if isinstance(other, str):
            tb = self.engine.acl_table(other)
            if other not in self.by_name or tb < 0:
                raise ClsError("acl diff: no ACL %r" % (other,))
        else:
            tmp = self.engine.put_table("acl_diff candidate", list(other))
            tb = tmp
        try:
            r = self.engine.table_diff(tid, tb, af=af, rec_cap=0)
            r = self.engine.table_diff(tid, tb, af=af, rec_cap=r["n_rec"])
        finally:
            if tmp is not None:
                self.engine.del_table(tmp)

        def ip(a):
            return "%d.%d.%d.%d" % (a >> 24, a >> 16 & 255, a >> 8 & 255, a & 255)

        def side(cells, wit):
            return {k: (int(cells[k]), (ip(int(w["src"])), ip(int(w["dst"])), int(w["proto"]), int(w["dport"])))
                    for k, w in enumerate(wit) if w["live"]}
        recs = [((ip(int(c["src_lo"])), ip(int(c["src_hi"])), ip(int(c["dst_lo"])), ip(int(c["dst_hi"]))),
                 int(c["proto"]), int(c["port_lo"]), int(c["port_hi"]), int(c["was"]), int(c["now"]),
                 int(c["rule_a"]), int(c["rule_b"])) for c in r["records"]]
        return {"equal": r["equal"], "n_diff": r["n_diff"], "n_cells": r["n_cells"], "pairs": r["pairs"].tolist(),
                "records": recs, "rules_a": side(r["cells_a"], r["wit_a"]), "rules_b": side(r["cells_b"], r["wit_b"])}

    def acl_needed(self, acl_name: str, keep=()):
        """Which rules an installed ACL actually needs (Engine.table_need over
        the ACL's compiled table; the reference has no such call).  Returns a
        dict: ``dead``, the rules no packet terminates at; ``redundant``, the
        live rules whose packets all get the same ACLAction from the rest of
        the list once the rule alone is gone; ``free``, the dead and
        redundant rules that can be deleted TOGETHER without changing a
        verdict (redundant rules are not jointly removable in general: of two
        equal PERMITs each is redundant given the other); ``needed``, rule
        index -> (src string, dst string, protocol, dport, after, fall): the
        least packet whose action changes without the rule, the action it
        then gets and the rule that then takes it (the rule count: the default
        DENY); ``default_reachable``.  ``keep``: rules never reported free.
        The sweep covers the IPv4 packet space only: a rule with an IPv6
        network is reported dead.  Raises ClsError for an unknown name."""
        tid = self.engine.acl_table(acl_name)
        if acl_name not in self.by_name or tid < 0:
            raise ClsError("acl needed: no ACL %r" % (acl_name,))
        r = self.engine.table_need(tid)
        n = len(r["need"])
        keep = set(int(k) for k in keep)

        def ip(a):
            return "%d.%d.%d.%d" % (a >> 24, a >> 16 & 255, a >> 8 & 255, a & 255)
        needed = {k: (ip(int(w["src"])), ip(int(w["dst"])), int(w["proto"]), int(w["dport"]), int(w["after"]) & 3,
                      int(w["fall"])) for k, w in enumerate(r["witness"]) if w["after"] & 0x80}
        return {"dead": [k for k in range(n) if r["need"][k] == _abi.NEED_DEAD],
                "redundant": [k for k in range(n) if r["need"][k] == _abi.NEED_REDUNDANT],
                "free": [k for k in range(n) if r["free"][k] and k not in keep], "needed": needed,
                "default_reachable": bool(r["first"][n])}

    def acl_minimize(self, acl_name: str, keep=(), keep_v6: bool = True, max_rounds: int = 64):
        """A smaller rule list with the same ACLAction for every IPv4 packet:
        (kept rule indices, removed indices per round).  Computes only --
        nothing is installed.  Rounds of Engine.table_need with a growing
        ``skip`` (minimize_rounds): each round removes every free rule outside
        ``keep``, until no rule outside ``keep`` is dead or redundant or
        ``max_rounds`` is reached (a rule that can only fall to a redundant
        rule pinned by ``keep`` stays).  The result is then checked with
        Engine.table_diff, the original against the reduced list, and ClsError
        is raised if they are not equal.  ``keep_v6`` pins every rule with an
        IPv6 (family-16) source or destination network: the IPv4 sweep sees
        those as dead, and they exist for packets the sweep does not cover."""
        tid = self.engine.acl_table(acl_name)
        acl = self.by_name.get(acl_name)
        if acl is None or tid < 0:
            raise ClsError("acl minimize: no ACL %r" % (acl_name,))
        rules = list(acl.rules)
        pinned = set(int(k) for k in keep) | (set(v6_rules(rules)) if keep_v6 else set())
        kept, rounds = minimize_rounds(lambda skip: self.engine.table_need(tid, skip=skip), len(rules), pinned,
                                       max_rounds)
        if rounds:
            tmp = self.engine.put_table("acl_minimize result", [rules[k] for k in kept])
            try:
                d = self.engine.table_diff(tid, tmp, rec_cap=0)
            finally:
                self.engine.del_table(tmp)
            if not d["equal"]:
                raise ClsError("acl minimize: the reduced list of %r differs on %d cells" % (acl_name, d["n_diff"]))
        return kept, rounds

    def connection_matrix_diff(self, pods, probes, base, count: bool = False):
        """connection_matrix against a baseline: (matrix, changes), matrix
        what connection_matrix(pods, probes) returns and changes the cells
        where it differs from ``base`` -- a [len(probes), len(pods),
        len(pods)] uint8 array, such as the matrix of an earlier commit -- as
        (probe index, src pod, dst pod, was, now) in cell order over ``pods``.
        One engine call (Engine.reach_diff) over the resolvable endpoints,
        which sees ``base`` restricted to them; the rows and columns of the
        pods left out are compared here against CONN_FAILURE."""
        base = np.asarray(base, np.uint8)
        if base.shape != (len(probes), len(pods), len(pods)):
            raise ClsError("connection matrix diff: base must have shape (probes, pods, pods)")
        out = np.full(base.shape, CONN_FAILURE, np.uint8)
        eps = self._matrix_endpoints(pods)
        cells = []                                  # (probe, src, dst, was, now), indices into pods
        if eps and probes:
            addrs = self._matrix_addrs(eps)
            pr = np.array(probes, np.int64).reshape(-1, 3)
            at = np.array([e[0] for e in eps])
            sub = np.ascontiguousarray(base[:, at[:, None], at[None, :]])
            r = self.engine.reach_diff([e[1] for e in eps], addrs, pr[:, 0], pr[:, 1], pr[:, 2], sub, count=count,
                                       trans=False, changed=False)
            out[:, at[:, None], at[None, :]] = r.verdicts
            cells = [(int(c["probe"]), int(at[c["src"]]), int(at[c["dst"]]), int(c["was"]), int(c["now"]))
                     for c in r.changes]
        # the pods left out: every cell of their rows and columns is CONN_FAILURE
        rest = np.ones(len(pods), bool)
        rest[[e[0] for e in eps]] = False
        outside = rest[:, None] | rest[None, :]
        cells += [(int(p), int(s), int(d), int(base[p, s, d]), CONN_FAILURE)
                  for p, s, d in np.argwhere((base != CONN_FAILURE) & outside[None])]
        cells.sort(key=lambda c: c[:3])
        return out, [(p, pods[s], pods[d], was, now) for p, s, d, was, now in cells]

    def connection_pod_to_pod(self, src_pod, dst_pod, proto, sport, dport):
        return self.connection_batch([("ConnectionPodToPod", (src_pod, dst_pod, proto, sport, dport))])[0]

    def connection_pod_to_internet(self, src_pod, dst_ip, proto, sport, dport):
        return self.connection_batch([("ConnectionPodToInternet", (src_pod, dst_ip, proto, sport, dport))])[0]

    def connection_internet_to_pod(self, src_ip, dst_pod, proto, sport, dport):
        return self.connection_batch([("ConnectionInternetToPod", (src_ip, dst_pod, proto, sport, dport))])[0]
