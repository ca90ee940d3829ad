// Package contivcls binds the MI355X batched first-match ACL classifier
// (include/contivcls.h, vpp_amd/libcontivcls.so) for the Contiv-VPP Go host.
//
// It is a drop-in for mock/aclengine.MockACLEngine
// (mock/aclengine/aclengine_mock.go:94-728): the same method set, the same
// verdict enums, the same error behaviour, with the ACL evaluation moved to
// the GPU and two batched entry points added (ClassifyBatch, ConnectionBatch).
//
// UNTESTED: the build image of this repository has no Go toolchain (SURVEY
// 8(c)), so this file has never been compiled.  The Python host
// (vpp_amd/engine.py, class ACLEngine) calls exactly the same C symbols in
// the same order and is what the parity tests exercise; keep the two in step.
//
// Go 1.9 (the reference's toolchain, .travis.yml:7-8): no runtime.Pinner,
// no unsafe.Slice, no post-1.9 library call.  Ownership (cgo rule): every
// pointer handed to the C ABI is valid only for the duration of the call;
// the engine deep-copies rules and keeps no caller pointer.  Packet and
// connection arrays go to the static C shims of include/contivcls_go.h as
// one scalar pointer per slice (pointer-free Go memory, which cgo allows for
// the call), and the shims build the ABI's SoA records on the C stack -- a
// Go value holding Go pointers never crosses.  Rule records hold only C
// strings (C.CString).  The shims themselves run on the GPU in
// tests/test_gpu_go_shims.py (go/shimtest/shimtest.c, gcc).
package contivcls

/*
#cgo CFLAGS: -I${SRCDIR}/../../include
#cgo LDFLAGS: -L${SRCDIR}/../../vpp_amd -lcontivcls -Wl,-rpath,${SRCDIR}/../../vpp_amd
#include <stdlib.h>
#include "contivcls_go.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"net"
	"strings"
	"sync"
	"unsafe"

	"github.com/contiv/vpp/mock/aclengine"
	"github.com/contiv/vpp/mock/localclient"
	"github.com/contiv/vpp/plugins/contiv"
	podmodel "github.com/contiv/vpp/plugins/ksr/model/pod"
	vpp_acl "github.com/ligato/vpp-agent/plugins/defaultplugins/common/model/acl"
)

// ACLAction values of evalACL (aclengine_mock.go:63-77) as the C ABI returns
// them per packet.
const (
	ACLDeny    = uint8(C.CLS_ACL_DENY)
	ACLPermit  = uint8(C.CLS_ACL_PERMIT)
	ACLReflect = uint8(C.CLS_ACL_REFLECT)
	ACLFailure = uint8(C.CLS_ACL_FAILURE)
)

// Engine replaces MockACLEngine.  The Go side keeps the pod registry and the
// installed protobufs (DumpACLs returns them); interface bindings and the
// compiled tables live in the C engine.
type Engine struct {
	sync.Mutex
	e      *C.cls_engine
	Contiv contiv.API

	pods   map[podmodel.ID]*podConfig
	byName map[string]*vpp_acl.AccessLists_Acl
}

type podConfig struct {
	ip          net.IP
	anotherNode bool
}

// New replaces NewMockACLEngine (aclengine_mock.go:124).  device: HIP device
// ordinal, -1 for the current one.
func New(c contiv.API, device int) (*Engine, error) {
	return NewMulti(c, []int{device})
}

// NewMulti: one engine over several devices (SURVEY 8(e)).  Every table is
// compiled once and replicated to every device; Batch packets shard over the
// devices; over distinct devices the hit counters of ClassifyBatchDevice are
// merged by the library's RCCL all-reduce over xGMI.
func NewMulti(c contiv.API, devices []int) (*Engine, error) {
	// the library this binding was written against (include/contivcls.h)
	if v := C.cls_abi_version(); v != C.clsg_abi_version() {
		return nil, fmt.Errorf("contivcls: library ABI %d, binding ABI %d", int(v), int(C.clsg_abi_version()))
	}
	if len(devices) == 0 {
		return nil, errors.New("contivcls: no device")
	}
	var e *C.cls_engine
	dl := make([]C.int, len(devices)) // pointer-free Go memory: the shim builds cls_config
	for i, d := range devices {
		dl[i] = C.int(d)
	}
	switch rc := C.clsg_engine_create(&dl[0], C.uint32_t(len(dl)), &e); rc {
	case C.CLS_OK:
	default:
		return nil, errors.New("contivcls: no usable gfx950 device")
	}
	return &Engine{e: e, Contiv: c, pods: map[podmodel.ID]*podConfig{},
		byName: map[string]*vpp_acl.AccessLists_Acl{}}, nil
}

// Close releases the engine and its device memory.
func (en *Engine) Close() {
	en.Lock()
	defer en.Unlock()
	if en.e != nil {
		C.cls_engine_destroy(en.e)
		en.e = nil
	}
}

func (en *Engine) lastErr() error { return errors.New(C.GoString(C.cls_last_error(en.e))) }

// cstrs frees the C strings a call borrowed.
type cstrs []*C.char

func (s *cstrs) add(v string) *C.char {
	p := C.CString(v)
	*s = append(*s, p)
	return p
}

func (s cstrs) free() {
	for _, p := range s {
		C.free(unsafe.Pointer(p))
	}
}

// flatten turns the protobuf rules into cls_rule records.  Presence bits
// carry the nil-ness of every sub-message evalACL looks at
// (aclengine_mock.go:481-664); the CIDR strings go verbatim and the engine
// parses them with Go 1.9 net.ParseCIDR semantics, so unparsable strings give
// the same FAILURE verdicts.  A rule with nil Matches (a panic in evalACL) is
// rejected by cls_table_put / cls_acl_put with CLS_E_INVAL.
func flatten(acl *vpp_acl.AccessLists_Acl, strs *cstrs) []C.cls_rule {
	rules := make([]C.cls_rule, len(acl.Rules))
	for i, r := range acl.Rules {
		c := &rules[i]
		if r.Actions != nil {
			c.flags |= C.CLS_R_ACTIONS
			c.acl_action = C.int32_t(r.Actions.AclAction)
		}
		m := r.Matches
		if m == nil {
			continue
		}
		c.flags |= C.CLS_R_MATCHES
		if m.MacipRule != nil {
			c.flags |= C.CLS_R_MACIP
		}
		ip := m.IpRule
		if ip == nil {
			continue
		}
		c.flags |= C.CLS_R_IPRULE
		if ip.Ip != nil {
			c.flags |= C.CLS_R_IP
			c.src_network = strs.add(ip.Ip.SourceNetwork)
			c.dst_network = strs.add(ip.Ip.DestinationNetwork)
		}
		if ip.Other != nil {
			c.flags |= C.CLS_R_OTHER
		}
		if t := ip.Tcp; t != nil {
			c.flags |= C.CLS_R_TCP
			if p := t.SourcePortRange; p != nil {
				c.flags |= C.CLS_R_TCP_SRC
				c.tcp_src_lo, c.tcp_src_hi = C.uint32_t(p.LowerPort), C.uint32_t(p.UpperPort)
			}
			if p := t.DestinationPortRange; p != nil {
				c.flags |= C.CLS_R_TCP_DST
				c.tcp_dst_lo, c.tcp_dst_hi = C.uint32_t(p.LowerPort), C.uint32_t(p.UpperPort)
			}
		}
		if u := ip.Udp; u != nil {
			c.flags |= C.CLS_R_UDP
			if p := u.SourcePortRange; p != nil {
				c.flags |= C.CLS_R_UDP_SRC
				c.udp_src_lo, c.udp_src_hi = C.uint32_t(p.LowerPort), C.uint32_t(p.UpperPort)
			}
			if p := u.DestinationPortRange; p != nil {
				c.flags |= C.CLS_R_UDP_DST
				c.udp_dst_lo, c.udp_dst_hi = C.uint32_t(p.LowerPort), C.uint32_t(p.UpperPort)
			}
		}
		if ic := ip.Icmp; ic != nil {
			c.flags |= C.CLS_R_ICMP
			if ic.Icmpv6 {
				c.flags |= C.CLS_R_ICMPV6
			}
			if p := ic.IcmpCodeRange; p != nil {
				c.flags |= C.CLS_R_ICMP_CODE
				c.icmp_code_first, c.icmp_code_last = C.uint32_t(p.First), C.uint32_t(p.Last)
			}
			if p := ic.IcmpTypeRange; p != nil {
				c.flags |= C.CLS_R_ICMP_TYPE
				c.icmp_type_first, c.icmp_type_last = C.uint32_t(p.First), C.uint32_t(p.Last)
			}
		}
	}
	return rules
}

// RegisterPod replaces MockACLEngine.RegisterPod (aclengine_mock.go:144-148).
func (en *Engine) RegisterPod(pod podmodel.ID, podIP string, anotherNode bool) {
	en.Lock()
	defer en.Unlock()
	en.pods[pod] = &podConfig{ip: net.ParseIP(podIP), anotherNode: anotherNode}
}

// ApplyTxn replaces MockACLEngine.ApplyTxn (aclengine_mock.go:151-198): the
// engine is the onCommit of the txn tracker (mock/localclient/txn.go:120-131).
// Like the reference, an error aborts mid-transaction with no rollback.
func (en *Engine) ApplyTxn(txn *localclient.Txn) error {
	en.Lock()
	defer en.Unlock()
	if txn == nil {
		return errors.New("txn is nil")
	}
	if txn.DefaultPluginsDataChangeTxn != nil || txn.DefaultPluginsDataResyncTxn != nil {
		return errors.New("defaultplugins txn is not supported")
	}
	if txn.LinuxDataResyncTxn != nil {
		return errors.New("linux resync txn is not supported")
	}
	if txn.LinuxDataChangeTxn == nil {
		return errors.New("linux data change txn is nil")
	}
	for _, op := range txn.LinuxDataChangeTxn.Ops {
		if !strings.HasPrefix(op.Key, vpp_acl.KeyPrefix()) {
			return errors.New("non-ACL changed in txn")
		}
		if op.Value == nil {
			name := strings.TrimPrefix(op.Key, vpp_acl.KeyPrefix())
			if err := en.delACL(name); err != nil {
				return err
			}
			continue
		}
		acl, ok := op.Value.(*vpp_acl.AccessLists_Acl)
		if !ok {
			return errors.New("failed to cast ACL value")
		}
		if err := en.putACL(acl); err != nil {
			return err
		}
	}
	return nil
}

// putACL: ACLConfig.PutACL (aclengine_mock.go:699-728) in the C engine
// (empty Interfaces is an error there too; a re-put of equal rules keeps the
// compiled table and only moves the bindings).
func (en *Engine) putACL(acl *vpp_acl.AccessLists_Acl) error {
	var strs cstrs
	defer strs.free()
	rules := flatten(acl, &strs)
	var ing, eg []*C.char
	if acl.Interfaces != nil {
		for _, s := range acl.Interfaces.Ingress {
			ing = append(ing, strs.add(s))
		}
		for _, s := range acl.Interfaces.Egress {
			eg = append(eg, strs.add(s))
		}
	}
	var rp *C.cls_rule
	if len(rules) > 0 {
		rp = &rules[0]
	}
	var ip, ep **C.char
	if len(ing) > 0 {
		ip = &ing[0]
	}
	if len(eg) > 0 {
		ep = &eg[0]
	}
	if rc := C.cls_acl_put(en.e, strs.add(acl.AclName), rp, C.uint32_t(len(rules)), ip, C.uint32_t(len(ing)),
		ep, C.uint32_t(len(eg))); rc != C.CLS_OK {
		return en.lastErr()
	}
	en.byName[acl.AclName] = acl
	return nil
}

// delACL: ACLConfig.DelACL (aclengine_mock.go:680-696).
func (en *Engine) delACL(name string) error {
	var strs cstrs
	defer strs.free()
	if rc := C.cls_acl_del(en.e, strs.add(name)); rc != C.CLS_OK {
		return en.lastErr()
	}
	delete(en.byName, name)
	return nil
}

// DumpACLs replaces MockACLEngine.DumpACLs (aclengine_mock.go:201-206).
func (en *Engine) DumpACLs() (acls []*vpp_acl.AccessLists_Acl) {
	en.Lock()
	defer en.Unlock()
	for _, acl := range en.byName {
		acls = append(acls, acl)
	}
	return acls
}

// GetNumOfACLs replaces MockACLEngine.GetNumOfACLs (:209-212).
func (en *Engine) GetNumOfACLs() int {
	n, _ := en.counts()
	return n
}

// GetNumOfACLChanges replaces MockACLEngine.GetNumOfACLChanges (:237-240).
func (en *Engine) GetNumOfACLChanges() int {
	_, c := en.counts()
	return c
}

func (en *Engine) counts() (int, int) {
	en.Lock()
	defer en.Unlock()
	var n, c C.uint32_t
	C.cls_acl_counts(en.e, &n, &c)
	return int(n), int(c)
}

// aclOfTable: the installed protobuf whose compiled table the engine bound.
func (en *Engine) aclOfTable(tid C.int32_t) *vpp_acl.AccessLists_Acl {
	if tid < 0 {
		return nil
	}
	var strs cstrs
	defer strs.free()
	for name, acl := range en.byName {
		var id C.uint32_t
		if C.cls_acl_table(en.e, strs.add(name), &id) == C.CLS_OK && C.int32_t(id) == tid {
			return acl
		}
	}
	return nil
}

func (en *Engine) ifACLs(ifName string) (in, out C.int32_t) {
	var strs cstrs
	defer strs.free()
	var id C.uint32_t
	in, out = -1, -1
	if C.cls_if_id(en.e, strs.add(ifName), &id) == C.CLS_OK {
		C.cls_if_acls(en.e, id, &in, &out)
	}
	return in, out
}

// GetInboundACL replaces MockACLEngine.GetInboundACL (:215-219).
func (en *Engine) GetInboundACL(ifName string) *vpp_acl.AccessLists_Acl {
	en.Lock()
	defer en.Unlock()
	in, _ := en.ifACLs(ifName)
	return en.aclOfTable(in)
}

// GetOutboundACL replaces MockACLEngine.GetOutboundACL (:222-226).
func (en *Engine) GetOutboundACL(ifName string) *vpp_acl.AccessLists_Acl {
	en.Lock()
	defer en.Unlock()
	_, out := en.ifACLs(ifName)
	return en.aclOfTable(out)
}

// GetACLByName replaces MockACLEngine.GetACLByName (:228-234).
func (en *Engine) GetACLByName(aclName string) *vpp_acl.AccessLists_Acl {
	en.Lock()
	defer en.Unlock()
	return en.byName[aclName]
}

// Conn is one Connection* call for ConnectionBatch.  Kind selects the
// reference entry point; the fields it does not use are ignored.
type Conn struct {
	Kind           ConnKind
	SrcPod, DstPod podmodel.ID
	SrcIP, DstIP   string // ConnectionInternetToPod / ConnectionPodToInternet
	Protocol       aclengine.ProtocolType
	SrcPort        uint16
	DstPort        uint16
}

// ConnKind names the reference entry point of a Conn.
type ConnKind int

const (
	PodToPod      ConnKind = iota // ConnectionPodToPod (aclengine_mock.go:243-300)
	PodToInternet                 // ConnectionPodToInternet (:304-345)
	InternetToPod                 // ConnectionInternetToPod (:349-390)
)

// nodeOutputIf: the VXLAN BVI, else the main physical interface (:272-279).
func (en *Engine) nodeOutputIf() string {
	if ifName := en.Contiv.GetVxlanBVIIfName(); ifName != "" {
		return ifName
	}
	return en.Contiv.GetMainPhysicalIfName()
}

func (en *Engine) podIf(pod podmodel.ID, cfg *podConfig) (string, bool) {
	if cfg.anotherNode {
		ifName := en.nodeOutputIf()
		return ifName, ifName != ""
	}
	return en.Contiv.GetIfName(pod.Namespace, pod.Name)
}

// resolve: interfaces and addresses of a call, as the reference finds them
// before testConnection; ok == false is ConnActionFailure.
func (en *Engine) resolve(c *Conn) (srcIf, dstIf string, srcIP, dstIP net.IP, ok bool) {
	switch c.Kind {
	case PodToPod:
		s, d := en.pods[c.SrcPod], en.pods[c.DstPod]
		if s == nil || d == nil {
			return
		}
		var ok1, ok2 bool
		srcIf, ok1 = en.podIf(c.SrcPod, s)
		dstIf, ok2 = en.podIf(c.DstPod, d)
		return srcIf, dstIf, s.ip, d.ip, ok1 && ok2
	case PodToInternet:
		s := en.pods[c.SrcPod]
		if s == nil || s.anotherNode {
			return
		}
		var ok1 bool
		srcIf, ok1 = en.Contiv.GetIfName(c.SrcPod.Namespace, c.SrcPod.Name)
		dstIf, dstIP = en.nodeOutputIf(), net.ParseIP(c.DstIP)
		return srcIf, dstIf, s.ip, dstIP, ok1 && dstIf != "" && dstIP != nil
	default:
		d := en.pods[c.DstPod]
		if d == nil || d.anotherNode {
			return
		}
		var ok2 bool
		srcIf, srcIP = en.nodeOutputIf(), net.ParseIP(c.SrcIP)
		dstIf, ok2 = en.Contiv.GetIfName(c.DstPod.Namespace, c.DstPod.Name)
		return srcIf, dstIf, srcIP, d.ip, srcIf != "" && srcIP != nil && ok2
	}
}

// ConnectionBatch evaluates many Connection* calls in one GPU launch
// (testConnection, aclengine_mock.go:394-471, per call): the IPv4 layout when
// every endpoint is IPv4, else the 16-byte layout (IPv4 as IPv4-mapped, as
// Go's To4).  count: add every evalACL call's terminating rule to the tables'
// connection counters (cls_conn_counters).
func (en *Engine) ConnectionBatch(calls []Conn, count bool) ([]aclengine.ConnectionAction, error) {
	out, _, err := en.connections(calls, count, false)
	return out, err
}

// ConnectRules is ConnectionBatch with the trace (cls_connect_rules): besides
// every call's ConnectionAction, the rule at which each of testConnection's
// four evalACL calls ended -- what the reference logs per call
// (aclengine_mock.go:651-654) -- in its order: SYN through the source
// interface's inbound ACL, SYN through the destination's outbound, SYN-ACK
// through the destination's inbound, SYN-ACK through the source's outbound.
// Each entry is the rule's index in that ACL (GetInboundACL / GetOutboundACL
// of the interface), len(Rules) for the default DENY, or -1 when
// testConnection does not make the call or makes it on a nil ACL; a call that
// fails before testConnection has four -1.  No counters are touched.
func (en *Engine) ConnectRules(calls []Conn) ([]aclengine.ConnectionAction, [][4]int32, error) {
	return en.connections(calls, false, true)
}

func (en *Engine) connections(calls []Conn, count bool, trace bool) ([]aclengine.ConnectionAction, [][4]int32, error) {
	en.Lock()
	defer en.Unlock()
	out := make([]aclengine.ConnectionAction, len(calls))
	var rules [][4]int32
	if trace {
		rules = make([][4]int32, len(calls))
		for i := range rules {
			rules[i] = [4]int32{-1, -1, -1, -1}
		}
	}
	var idx []int
	var sif, dif []uint32
	var sip, dip []net.IP
	var proto []uint8
	var sport, dport []uint16
	var strs cstrs
	defer strs.free()
	ifID := map[string]uint32{}
	id := func(name string) uint32 {
		if v, ok := ifID[name]; ok {
			return v
		}
		var v C.uint32_t
		C.cls_if_id(en.e, strs.add(name), &v)
		ifID[name] = uint32(v)
		return uint32(v)
	}
	v4 := true
	for i := range calls {
		s, d, a, b, ok := en.resolve(&calls[i])
		if !ok {
			out[i] = aclengine.ConnActionFailure
			continue
		}
		idx = append(idx, i)
		sif, dif = append(sif, id(s)), append(dif, id(d))
		sip, dip = append(sip, a), append(dip, b)
		proto = append(proto, uint8(calls[i].Protocol))
		sport, dport = append(sport, calls[i].SrcPort), append(dport, calls[i].DstPort)
		v4 = v4 && a.To4() != nil && b.To4() != nil
	}
	n := len(idx)
	if n == 0 {
		return out, rules, nil
	}
	// every slice goes to the shim as its own pointer (pointer-free Go
	// memory); the shim builds cls_conn_soa on the C stack
	res := make([]uint8, n)
	var tr []int32 // the trace: four rules per evaluated connection
	if trace {
		tr = make([]int32, 4*n)
	}
	flags := C.uint32_t(0)
	if count {
		flags |= C.CLS_F_COUNT
	}
	var rc C.int
	if v4 {
		s4, d4 := make([]uint32, n), make([]uint32, n)
		for k := 0; k < n; k++ {
			a, b := sip[k].To4(), dip[k].To4()
			s4[k] = uint32(a[0])<<24 | uint32(a[1])<<16 | uint32(a[2])<<8 | uint32(a[3])
			d4[k] = uint32(b[0])<<24 | uint32(b[1])<<16 | uint32(b[2])<<8 | uint32(b[3])
		}
		if trace {
			rc = C.clsg_connect_rules_v4(en.e, (*C.uint32_t)(&sif[0]), (*C.uint32_t)(&dif[0]), (*C.uint32_t)(&s4[0]),
				(*C.uint32_t)(&d4[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), (*C.uint8_t)(&proto[0]),
				C.uint64_t(n), (*C.uint8_t)(&res[0]), (*C.int32_t)(&tr[0]), flags)
		} else {
			rc = C.clsg_connect_v4(en.e, (*C.uint32_t)(&sif[0]), (*C.uint32_t)(&dif[0]), (*C.uint32_t)(&s4[0]),
				(*C.uint32_t)(&d4[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), (*C.uint8_t)(&proto[0]),
				C.uint64_t(n), (*C.uint8_t)(&res[0]), flags)
		}
	} else {
		s16, d16 := make([]byte, 16*n), make([]byte, 16*n)
		for k := 0; k < n; k++ {
			a, b := sip[k].To16(), dip[k].To16()
			if a == nil || b == nil {
				return nil, nil, errors.New("connection endpoint is not an IPv4 or IPv6 address")
			}
			copy(s16[16*k:], a)
			copy(d16[16*k:], b)
		}
		if trace {
			rc = C.clsg_connect_rules_v16(en.e, (*C.uint32_t)(&sif[0]), (*C.uint32_t)(&dif[0]), (*C.uint8_t)(&s16[0]),
				(*C.uint8_t)(&d16[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), (*C.uint8_t)(&proto[0]),
				C.uint64_t(n), (*C.uint8_t)(&res[0]), (*C.int32_t)(&tr[0]), flags)
		} else {
			rc = C.clsg_connect_v16(en.e, (*C.uint32_t)(&sif[0]), (*C.uint32_t)(&dif[0]), (*C.uint8_t)(&s16[0]),
				(*C.uint8_t)(&d16[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), (*C.uint8_t)(&proto[0]),
				C.uint64_t(n), (*C.uint8_t)(&res[0]), flags)
		}
	}
	if rc != C.CLS_OK {
		return nil, nil, en.lastErr()
	}
	for k, i := range idx {
		out[i] = aclengine.ConnectionAction(res[k])
		if trace {
			copy(rules[i][:], tr[4*k:4*k+4])
		}
	}
	return out, rules, nil
}

// ConnectionPodToPod replaces MockACLEngine.ConnectionPodToPod (:243-300).
func (en *Engine) ConnectionPodToPod(srcPod podmodel.ID, dstPod podmodel.ID, protocol aclengine.ProtocolType,
	srcPort uint16, dstPort uint16) aclengine.ConnectionAction {
	return en.one(Conn{Kind: PodToPod, SrcPod: srcPod, DstPod: dstPod, Protocol: protocol,
		SrcPort: srcPort, DstPort: dstPort})
}

// ConnectionPodToInternet replaces MockACLEngine.ConnectionPodToInternet (:304-345).
func (en *Engine) ConnectionPodToInternet(srcPod podmodel.ID, dstIP string, protocol aclengine.ProtocolType,
	srcPort uint16, dstPort uint16) aclengine.ConnectionAction {
	return en.one(Conn{Kind: PodToInternet, SrcPod: srcPod, DstIP: dstIP, Protocol: protocol,
		SrcPort: srcPort, DstPort: dstPort})
}

// ConnectionInternetToPod replaces MockACLEngine.ConnectionInternetToPod (:349-390).
func (en *Engine) ConnectionInternetToPod(srcIP string, dstPod podmodel.ID, protocol aclengine.ProtocolType,
	srcPort uint16, dstPort uint16) aclengine.ConnectionAction {
	return en.one(Conn{Kind: InternetToPod, SrcIP: srcIP, DstPod: dstPod, Protocol: protocol,
		SrcPort: srcPort, DstPort: dstPort})
}

func (en *Engine) one(c Conn) aclengine.ConnectionAction {
	res, err := en.ConnectionBatch([]Conn{c}, false)
	if err != nil {
		return aclengine.ConnActionFailure
	}
	return res[0]
}

// Probe is one (protocol, source port, destination port) question of a
// reachability matrix.
type Probe struct {
	Protocol aclengine.ProtocolType
	SrcPort  uint16
	DstPort  uint16
}

// Reach is the result of ReachMatrix over P probes and N pods: Verdicts[(p*N +
// s)*N + d] is what ConnectionPodToPod(pods[s], pods[d], probes[p]...)
// returns, Hist[p][a] the cells of probe p with ConnectionAction a, Allow[p*N
// + s] the pods that pods[s] reaches on probe p (ConnActionAllow).
type Reach struct {
	N, P     int
	Verdicts []aclengine.ConnectionAction
	Hist     [][4]uint64
	Allow    []uint32
}

// ReachMatrix answers what the reference's tests ask by looping
// ConnectionPodToPod over pods and ports (aclengine_mock.go:243-300) -- who
// reaches whom, on which probe -- in one engine call (cls_reach_matrix): the
// engine receives the pods' endpoints and the probes, never a row per cell.
// Pods that ConnectionPodToPod fails before testConnection (unregistered, no
// interface) stay out of the call: their rows and columns are
// ConnActionFailure.  The IPv4 layout when every endpoint is IPv4, else the
// 16-byte layout.  count: add every evalACL call's terminating rule to the
// tables' connection counters (ConnCounters): the rules left at zero are
// those no pod pair can hit.
func (en *Engine) ReachMatrix(pods []podmodel.ID, probes []Probe, count bool) (*Reach, error) {
	en.Lock()
	defer en.Unlock()
	N, P := len(pods), len(probes)
	out := &Reach{N: N, P: P, Verdicts: make([]aclengine.ConnectionAction, P*N*N), Hist: make([][4]uint64, P),
		Allow: make([]uint32, P*N)}
	for i := range out.Verdicts {
		out.Verdicts[i] = aclengine.ConnActionFailure
	}
	for p := range out.Hist {
		out.Hist[p][aclengine.ConnActionFailure] = uint64(N) * uint64(N)
	}
	var strs cstrs
	defer strs.free()
	var at []int // endpoint -> index in pods
	var ifs []uint32
	var ips []net.IP
	v4 := true
	for i, pod := range pods {
		cfg := en.pods[pod]
		if cfg == nil {
			continue
		}
		ifName, ok := en.podIf(pod, cfg)
		if !ok {
			continue
		}
		var v C.uint32_t
		C.cls_if_id(en.e, strs.add(ifName), &v)
		at, ifs, ips = append(at, i), append(ifs, uint32(v)), append(ips, cfg.ip)
		v4 = v4 && cfg.ip.To4() != nil
	}
	n := len(at)
	if n == 0 || P == 0 {
		return out, nil
	}
	proto, sport, dport := make([]uint8, P), make([]uint16, P), make([]uint16, P)
	for p, q := range probes {
		proto[p], sport[p], dport[p] = uint8(q.Protocol), q.SrcPort, q.DstPort
	}
	// every slice goes to the shim as its own pointer (pointer-free Go
	// memory); the shim builds cls_reach_spec on the C stack
	res, hist, allow := make([]uint8, P*n*n), make([]uint64, 4*P), make([]uint32, P*n)
	flags := C.uint32_t(0)
	if count {
		flags |= C.CLS_F_COUNT
	}
	var rc C.int
	if v4 {
		a4 := make([]uint32, n)
		for k := 0; k < n; k++ {
			a := ips[k].To4()
			a4[k] = uint32(a[0])<<24 | uint32(a[1])<<16 | uint32(a[2])<<8 | uint32(a[3])
		}
		rc = C.clsg_reach_matrix_v4(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint32_t)(&a4[0]), C.uint32_t(n),
			(*C.uint8_t)(&proto[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), C.uint32_t(P),
			(*C.uint8_t)(&res[0]), (*C.uint64_t)(&hist[0]), (*C.uint32_t)(&allow[0]), flags)
	} else {
		a16 := make([]byte, 16*n)
		for k := 0; k < n; k++ {
			a := ips[k].To16()
			if a == nil {
				return nil, errors.New("connection endpoint is not an IPv4 or IPv6 address")
			}
			copy(a16[16*k:], a)
		}
		rc = C.clsg_reach_matrix_v16(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint8_t)(&a16[0]), C.uint32_t(n),
			(*C.uint8_t)(&proto[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), C.uint32_t(P),
			(*C.uint8_t)(&res[0]), (*C.uint64_t)(&hist[0]), (*C.uint32_t)(&allow[0]), flags)
	}
	if rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	for p := 0; p < P; p++ {
		for a := 0; a < 4; a++ {
			out.Hist[p][a] = hist[4*p+a]
		}
		// the pods left out: N*N - n*n more failures
		out.Hist[p][aclengine.ConnActionFailure] += uint64(N)*uint64(N) - uint64(n)*uint64(n)
		for s := 0; s < n; s++ {
			out.Allow[p*N+at[s]] = allow[p*n+s]
			for d := 0; d < n; d++ {
				out.Verdicts[(p*N+at[s])*N+at[d]] = aclengine.ConnectionAction(res[(p*n+s)*n+d])
			}
		}
	}
	return out, nil
}

// ReachChange is one changed cell of ReachDiff: the probe's index, the source
// and destination pods' indices, the baseline's byte and the new action.
type ReachChange struct {
	Probe, Src, Dst int
	Was, Now        aclengine.ConnectionAction
}

// ReachDiff answers "what connectivity did this commit change?": the matrix
// ReachMatrix(pods, probes) would return now, and the cells in which it
// differs from base -- the Verdicts of an earlier ReachMatrix over the same
// pods and probes -- in cell order, compared on the device in the same engine
// call (cls_reach_diff): only the changed cells' records come back besides
// the matrix.  The engine sees base restricted to the pods that reach
// testConnection; the rows and columns of the others are compared here
// against ConnActionFailure.
func (en *Engine) ReachDiff(pods []podmodel.ID, probes []Probe, base []aclengine.ConnectionAction,
	count bool) (*Reach, []ReachChange, error) {
	en.Lock()
	defer en.Unlock()
	N, P := len(pods), len(probes)
	if len(base) != P*N*N {
		return nil, nil, errors.New("ReachDiff: base must hold P*N*N verdicts")
	}
	out := &Reach{N: N, P: P, Verdicts: make([]aclengine.ConnectionAction, P*N*N), Hist: make([][4]uint64, P),
		Allow: make([]uint32, P*N)}
	for i := range out.Verdicts {
		out.Verdicts[i] = aclengine.ConnActionFailure
	}
	for p := range out.Hist {
		out.Hist[p][aclengine.ConnActionFailure] = uint64(N) * uint64(N)
	}
	var strs cstrs
	defer strs.free()
	var at []int // endpoint -> index in pods
	var ifs []uint32
	var ips []net.IP
	inside := make([]bool, N)
	v4 := true
	for i, pod := range pods {
		cfg := en.pods[pod]
		if cfg == nil {
			continue
		}
		ifName, ok := en.podIf(pod, cfg)
		if !ok {
			continue
		}
		var v C.uint32_t
		C.cls_if_id(en.e, strs.add(ifName), &v)
		at, ifs, ips = append(at, i), append(ifs, uint32(v)), append(ips, cfg.ip)
		inside[i] = true
		v4 = v4 && cfg.ip.To4() != nil
	}
	n := len(at)
	var inner []ReachChange // the engine's records, over pods
	if n > 0 && P > 0 {
		proto, sport, dport := make([]uint8, P), make([]uint16, P), make([]uint16, P)
		for p, q := range probes {
			proto[p], sport[p], dport[p] = uint8(q.Protocol), q.SrcPort, q.DstPort
		}
		// every slice goes to the shim as its own pointer (pointer-free Go
		// memory); the shim builds both structs on the C stack
		sub := make([]uint8, P*n*n)
		for p := 0; p < P; p++ {
			for s := 0; s < n; s++ {
				for d := 0; d < n; d++ {
					sub[(p*n+s)*n+d] = uint8(base[(p*N+at[s])*N+at[d]])
				}
			}
		}
		res, hist, allow := make([]uint8, P*n*n), make([]uint64, 4*P), make([]uint32, P*n)
		rec := make([]uint32, 4*P*n*n) // 16-byte records: probe, src, dst, was | now << 8
		var total C.uint64_t
		flags := C.uint32_t(0)
		if count {
			flags |= C.CLS_F_COUNT
		}
		var rc C.int
		if v4 {
			a4 := make([]uint32, n)
			for k := 0; k < n; k++ {
				a := ips[k].To4()
				a4[k] = uint32(a[0])<<24 | uint32(a[1])<<16 | uint32(a[2])<<8 | uint32(a[3])
			}
			rc = C.clsg_reach_diff_v4(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint32_t)(&a4[0]), C.uint32_t(n),
				(*C.uint8_t)(&proto[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), C.uint32_t(P),
				(*C.uint8_t)(&sub[0]), (*C.uint8_t)(&res[0]), (*C.uint64_t)(&hist[0]), (*C.uint32_t)(&allow[0]),
				unsafe.Pointer(&rec[0]), C.uint64_t(P*n*n), &total, nil, nil, flags)
		} else {
			a16 := make([]byte, 16*n)
			for k := 0; k < n; k++ {
				a := ips[k].To16()
				if a == nil {
					return nil, nil, errors.New("connection endpoint is not an IPv4 or IPv6 address")
				}
				copy(a16[16*k:], a)
			}
			rc = C.clsg_reach_diff_v16(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint8_t)(&a16[0]), C.uint32_t(n),
				(*C.uint8_t)(&proto[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), C.uint32_t(P),
				(*C.uint8_t)(&sub[0]), (*C.uint8_t)(&res[0]), (*C.uint64_t)(&hist[0]), (*C.uint32_t)(&allow[0]),
				unsafe.Pointer(&rec[0]), C.uint64_t(P*n*n), &total, nil, nil, flags)
		}
		if rc != C.CLS_OK {
			return nil, nil, en.lastErr()
		}
		for p := 0; p < P; p++ {
			for a := 0; a < 4; a++ {
				out.Hist[p][a] = hist[4*p+a]
			}
			// the pods left out: N*N - n*n more failures
			out.Hist[p][aclengine.ConnActionFailure] += uint64(N)*uint64(N) - uint64(n)*uint64(n)
			for s := 0; s < n; s++ {
				out.Allow[p*N+at[s]] = allow[p*n+s]
				for d := 0; d < n; d++ {
					out.Verdicts[(p*N+at[s])*N+at[d]] = aclengine.ConnectionAction(res[(p*n+s)*n+d])
				}
			}
		}
		for k := 0; k < int(total); k++ {
			r := rec[4*k : 4*k+4]
			inner = append(inner, ReachChange{Probe: int(r[0]), Src: at[r[1]], Dst: at[r[2]],
				Was: aclengine.ConnectionAction(r[3] & 0xFF), Now: aclengine.ConnectionAction(r[3] >> 8 & 0xFF)})
		}
	}
	if n == N {
		return out, inner, nil
	}
	// merge, in cell order, with the cells of the pods left out that the
	// baseline did not already hold as failures (at is ascending, so the
	// engine's records are in cell order over pods too)
	var changes []ReachChange
	k := 0
	for p := 0; p < P; p++ {
		for s := 0; s < N; s++ {
			for d := 0; d < N; d++ {
				if inside[s] && inside[d] {
					if k < len(inner) && inner[k].Probe == p && inner[k].Src == s && inner[k].Dst == d {
						changes = append(changes, inner[k])
						k++
					}
				} else if was := base[(p*N+s)*N+d]; was != aclengine.ConnActionFailure {
					changes = append(changes, ReachChange{Probe: p, Src: s, Dst: d, Was: was,
						Now: aclengine.ConnActionFailure})
				}
			}
		}
	}
	return out, changes, nil
}

// PortRange is one maximal range of ReachPorts: ConnectionPodToPod(pods[Src],
// pods[Dst], protocol, srcPort, port) returns Action for every destination
// port in [Lo, Hi].
type PortRange struct {
	Src, Dst int
	Lo, Hi   uint16
	Action   aclengine.ConnectionAction
}

// ReachPorts answers "on which destination ports does pod s reach pod d?" for
// all 65,536 ports in one engine call (cls_reach_ports): the engine evaluates
// one representative port per port class of the bound ACLs and returns only
// the maximal ranges, in (Src, Dst, Lo) order, the ranges of a pair covering
// 0..65535; runs[s*N+d] is the number of ranges of the pair.  Pods that
// ConnectionPodToPod fails before testConnection stay out of the call: their
// pairs are the one range 0..65535 of ConnActionFailure.
func (en *Engine) ReachPorts(pods []podmodel.ID, protocol aclengine.ProtocolType, srcPort uint16) ([]PortRange,
	[]uint32, error) {
	en.Lock()
	defer en.Unlock()
	N := len(pods)
	runs := make([]uint32, N*N)
	for i := range runs {
		runs[i] = 1
	}
	var strs cstrs
	defer strs.free()
	var at []int // endpoint -> index in pods
	var ifs []uint32
	var ips []net.IP
	inside := make([]bool, N)
	v4 := true
	for i, pod := range pods {
		cfg := en.pods[pod]
		if cfg == nil {
			continue
		}
		ifName, ok := en.podIf(pod, cfg)
		if !ok {
			continue
		}
		var v C.uint32_t
		C.cls_if_id(en.e, strs.add(ifName), &v)
		at, ifs, ips = append(at, i), append(ifs, uint32(v)), append(ips, cfg.ip)
		inside[i] = true
		v4 = v4 && cfg.ip.To4() != nil
	}
	n := len(at)
	var rec []uint32 // 16-byte records: src, dst, lo | hi << 16, action
	total := 0
	if n > 0 {
		a4 := make([]uint32, n)
		a16 := make([]byte, 16*n)
		for k := 0; k < n; k++ {
			if v4 {
				a := ips[k].To4()
				a4[k] = uint32(a[0])<<24 | uint32(a[1])<<16 | uint32(a[2])<<8 | uint32(a[3])
			} else {
				a := ips[k].To16()
				if a == nil {
					return nil, nil, errors.New("connection endpoint is not an IPv4 or IPv6 address")
				}
				copy(a16[16*k:], a)
			}
		}
		// every slice goes to the shim as its own pointer (pointer-free Go
		// memory); the shim builds both structs on the C stack.  The ranges
		// are counted first, then fetched.
		inner := make([]uint32, n*n)
		var count C.uint64_t
		for pass := 0; pass < 2; pass++ {
			var buf unsafe.Pointer
			var irun *C.uint32_t
			if pass == 1 {
				rec = make([]uint32, 4*int(count))
				buf = unsafe.Pointer(&rec[0])
				irun = (*C.uint32_t)(&inner[0])
			}
			var rc C.int
			if v4 {
				rc = C.clsg_reach_ports_v4(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint32_t)(&a4[0]), C.uint32_t(n),
					C.uint8_t(protocol), C.uint16_t(srcPort), buf, count, &count, irun, nil, nil, nil, 0)
			} else {
				rc = C.clsg_reach_ports_v16(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint8_t)(&a16[0]), C.uint32_t(n),
					C.uint8_t(protocol), C.uint16_t(srcPort), buf, count, &count, irun, nil, nil, nil, 0)
			}
			if rc != C.CLS_OK {
				return nil, nil, en.lastErr()
			}
		}
		total = len(rec) / 4
		if int(count) < total { // (the bindings cannot change under the lock)
			total = int(count)
		}
		for s := 0; s < n; s++ {
			for d := 0; d < n; d++ {
				runs[at[s]*N+at[d]] = inner[s*n+d]
			}
		}
	}
	// merge, in pair order, with the pairs of the pods left out (at is
	// ascending, so the engine's records are in pair order over pods too)
	var out []PortRange
	k := 0
	for s := 0; s < N; s++ {
		for d := 0; d < N; d++ {
			if !inside[s] || !inside[d] {
				out = append(out, PortRange{Src: s, Dst: d, Lo: 0, Hi: 65535, Action: aclengine.ConnActionFailure})
				continue
			}
			for k < total && at[rec[4*k]] == s && at[rec[4*k+1]] == d {
				out = append(out, PortRange{Src: s, Dst: d, Lo: uint16(rec[4*k+2] & 0xFFFF),
					Hi: uint16(rec[4*k+2] >> 16), Action: aclengine.ConnectionAction(rec[4*k+3] & 0xFF)})
				k++
			}
		}
	}
	return out, runs, nil
}

// HopsNone is the hop count of a pod that is not reached (CLS_HOPS_NONE).
const HopsNone = 255

// Hops is the result of ReachHops over N pods: Hops[s*N+d] is the least number
// of connections, each allowed under some probe, that lead from pods[s] to
// pods[d] through other pods of the list -- 0 for s == d, HopsNone when there
// is no such path within the hop limit; Reach[s] the pods s reaches (its blast
// radius), Exposed[d] the pods that reach d, Levels[h] the pairs h hops apart.
type Hops struct {
	N       int
	Hops    []uint8
	Reach   []uint32
	Exposed []uint32
	Levels  [256]uint64
}

// ReachHops answers "if pod s is compromised, what can it reach in any number
// of hops?" in one engine call (cls_reach_hops): the matrix of ReachMatrix's
// arguments is evaluated on the device, folded into an adjacency bitmap there
// and searched from every pod at once; only the hop counts come back.  maxHops
// bounds the paths (0: 254).  Pods that ConnectionPodToPod fails before
// testConnection stay out of the call: they reach nothing and nothing reaches
// them.
func (en *Engine) ReachHops(pods []podmodel.ID, probes []Probe, maxHops int) (*Hops, error) {
	en.Lock()
	defer en.Unlock()
	N, P := len(pods), len(probes)
	if maxHops < 0 || maxHops > 254 {
		return nil, errors.New("ReachHops: maxHops must be 0 .. 254")
	}
	out := &Hops{N: N, Hops: make([]uint8, N*N), Reach: make([]uint32, N), Exposed: make([]uint32, N)}
	for i := range out.Hops {
		out.Hops[i] = HopsNone
	}
	for s := 0; s < N; s++ {
		out.Hops[s*N+s] = 0
	}
	out.Levels[0] = uint64(N)
	out.Levels[HopsNone] = uint64(N)*uint64(N) - uint64(N)
	var strs cstrs
	defer strs.free()
	var at []int // endpoint -> index in pods
	var ifs []uint32
	var ips []net.IP
	v4 := true
	for i, pod := range pods {
		cfg := en.pods[pod]
		if cfg == nil {
			continue
		}
		ifName, ok := en.podIf(pod, cfg)
		if !ok {
			continue
		}
		var v C.uint32_t
		C.cls_if_id(en.e, strs.add(ifName), &v)
		at, ifs, ips = append(at, i), append(ifs, uint32(v)), append(ips, cfg.ip)
		v4 = v4 && cfg.ip.To4() != nil
	}
	n := len(at)
	if n == 0 || P == 0 {
		return out, nil
	}
	proto, sport, dport := make([]uint8, P), make([]uint16, P), make([]uint16, P)
	for p, q := range probes {
		proto[p], sport[p], dport[p] = uint8(q.Protocol), q.SrcPort, q.DstPort
	}
	// every slice goes to the shim as its own pointer (pointer-free Go
	// memory); the shim builds both structs on the C stack
	hops, reach, exposed, levels := make([]uint8, n*n), make([]uint32, n), make([]uint32, n), make([]uint64, 256)
	var rc C.int
	if v4 {
		a4 := make([]uint32, n)
		for k := 0; k < n; k++ {
			a := ips[k].To4()
			a4[k] = uint32(a[0])<<24 | uint32(a[1])<<16 | uint32(a[2])<<8 | uint32(a[3])
		}
		rc = C.clsg_reach_hops_v4(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint32_t)(&a4[0]), C.uint32_t(n),
			(*C.uint8_t)(&proto[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), C.uint32_t(P),
			C.uint32_t(maxHops), (*C.uint8_t)(&hops[0]), (*C.uint32_t)(&reach[0]), (*C.uint32_t)(&exposed[0]),
			(*C.uint64_t)(&levels[0]), nil, 0)
	} else {
		a16 := make([]byte, 16*n)
		for k := 0; k < n; k++ {
			a := ips[k].To16()
			if a == nil {
				return nil, errors.New("connection endpoint is not an IPv4 or IPv6 address")
			}
			copy(a16[16*k:], a)
		}
		rc = C.clsg_reach_hops_v16(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint8_t)(&a16[0]), C.uint32_t(n),
			(*C.uint8_t)(&proto[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), C.uint32_t(P),
			C.uint32_t(maxHops), (*C.uint8_t)(&hops[0]), (*C.uint32_t)(&reach[0]), (*C.uint32_t)(&exposed[0]),
			(*C.uint64_t)(&levels[0]), nil, 0)
	}
	if rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	for s := 0; s < n; s++ {
		out.Reach[at[s]], out.Exposed[at[s]] = reach[s], exposed[s]
		for d := 0; d < n; d++ {
			out.Hops[at[s]*N+at[d]] = hops[s*n+d]
		}
	}
	// the pods left out: N*N - n*n more pairs, all unreached but their diagonal
	for h := 1; h < HopsNone; h++ {
		out.Levels[h] = levels[h]
	}
	out.Levels[HopsNone] = levels[HopsNone] + uint64(N)*uint64(N) - uint64(n)*uint64(n) - uint64(N-n)
	return out, nil
}

// ClassNone is Quot[p][c][c] of a class with one member (CLS_CLASS_NONE).
const ClassNone = 255

// Classes is the result of ReachClasses over N pods and P probes: the
// connectivity map.  Class[i] is the class of pods[i], or -1 for a pod that
// ConnectionPodToPod fails before testConnection (it is in no class); pods of
// one class cannot be told apart by the probes: exchanging two of them leaves
// the matrix of ReachMatrix unchanged.  Classes are numbered by their first
// pod: Rep[c] is its index in pods, Size[c] the members.  Self[p*C+c] is the
// ConnectionAction of a member of c to itself, Quot[(p*C+a)*C+b] the one from
// any member of a to any member of b, and for a == b between two members of a
// (ClassNone when a has one member).
type Classes struct {
	N, P, C int
	Class   []int32
	Rep     []uint32
	Size    []uint32
	Self    []uint8
	Quot    []uint8
	Rounds  int
}

// ReachClasses summarises the matrix of ReachMatrix's arguments in one engine
// call (cls_reach_classes): the matrix is evaluated on the device and only the
// classes and the P x C x C quotient come back.  The call is made with room
// for 64 classes and once more with room for all when there are more.
func (en *Engine) ReachClasses(pods []podmodel.ID, probes []Probe) (*Classes, error) {
	en.Lock()
	defer en.Unlock()
	N, P := len(pods), len(probes)
	out := &Classes{N: N, P: P, Class: make([]int32, N)}
	for i := range out.Class {
		out.Class[i] = -1
	}
	var strs cstrs
	defer strs.free()
	var at []int // endpoint -> index in pods
	var ifs []uint32
	var ips []net.IP
	v4 := true
	for i, pod := range pods {
		cfg := en.pods[pod]
		if cfg == nil {
			continue
		}
		ifName, ok := en.podIf(pod, cfg)
		if !ok {
			continue
		}
		var v C.uint32_t
		C.cls_if_id(en.e, strs.add(ifName), &v)
		at, ifs, ips = append(at, i), append(ifs, uint32(v)), append(ips, cfg.ip)
		v4 = v4 && cfg.ip.To4() != nil
	}
	n := len(at)
	if n == 0 || P == 0 {
		return out, nil
	}
	proto, sport, dport := make([]uint8, P), make([]uint16, P), make([]uint16, P)
	for p, q := range probes {
		proto[p], sport[p], dport[p] = uint8(q.Protocol), q.SrcPort, q.DstPort
	}
	a4, a16 := make([]uint32, 1), make([]byte, 16)
	if v4 {
		a4 = make([]uint32, n)
		for k := 0; k < n; k++ {
			a := ips[k].To4()
			a4[k] = uint32(a[0])<<24 | uint32(a[1])<<16 | uint32(a[2])<<8 | uint32(a[3])
		}
	} else {
		a16 = make([]byte, 16*n)
		for k := 0; k < n; k++ {
			a := ips[k].To16()
			if a == nil {
				return nil, errors.New("connection endpoint is not an IPv4 or IPv6 address")
			}
			copy(a16[16*k:], a)
		}
	}
	// every slice goes to the shim as its own pointer (pointer-free Go
	// memory); the shim builds both structs on the C stack
	classes := make([]uint32, n)
	count := make([]uint32, 2) // C, rounds
	room := 64
	var rep, size []uint32
	var self, quot []uint8
	for turn := 0; turn < 2; turn++ {
		rep, size = make([]uint32, room), make([]uint32, room)
		self, quot = make([]uint8, P*room), make([]uint8, P*room*room)
		var rc C.int
		if v4 {
			rc = C.clsg_reach_classes_v4(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint32_t)(&a4[0]), C.uint32_t(n),
				(*C.uint8_t)(&proto[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), C.uint32_t(P),
				(*C.uint32_t)(&classes[0]), (*C.uint32_t)(&count[0]), C.uint64_t(room), (*C.uint32_t)(&rep[0]),
				(*C.uint32_t)(&size[0]), (*C.uint8_t)(&self[0]), (*C.uint8_t)(&quot[0]), nil,
				(*C.uint32_t)(&count[1]), 0)
		} else {
			rc = C.clsg_reach_classes_v16(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint8_t)(&a16[0]), C.uint32_t(n),
				(*C.uint8_t)(&proto[0]), (*C.uint16_t)(&sport[0]), (*C.uint16_t)(&dport[0]), C.uint32_t(P),
				(*C.uint32_t)(&classes[0]), (*C.uint32_t)(&count[0]), C.uint64_t(room), (*C.uint32_t)(&rep[0]),
				(*C.uint32_t)(&size[0]), (*C.uint8_t)(&self[0]), (*C.uint8_t)(&quot[0]), nil,
				(*C.uint32_t)(&count[1]), 0)
		}
		if rc != C.CLS_OK {
			return nil, en.lastErr()
		}
		if int(count[0]) <= room {
			break
		}
		room = int(count[0]) // the per-class outputs were left alone
	}
	nc := int(count[0])
	out.C, out.Rounds = nc, int(count[1])
	out.Rep, out.Size = make([]uint32, nc), size[:nc]
	for c := 0; c < nc; c++ {
		out.Rep[c] = uint32(at[rep[c]])
	}
	// (dense in C, whatever the room was)
	out.Self, out.Quot = self[:P*nc], quot[:P*nc*nc]
	for k := 0; k < n; k++ {
		out.Class[at[k]] = int32(classes[k])
	}
	return out, nil
}

// AddrRange is one maximal range of ReachExternal: for every IPv4 address a in
// [Lo, Hi] (host order), ConnectionPodToInternet(pods[Pod], a, probe) --
// Ingress false -- or ConnectionInternetToPod(a, pods[Pod], probe) -- Ingress
// true -- returns Action, probe being probes[Probe].
type AddrRange struct {
	Ingress    bool
	Probe, Pod int
	Lo, Hi     uint32
	Action     aclengine.ConnectionAction
}

// ReachExternal answers "which remote addresses can this pod talk to, and
// which can reach it?" for all of IPv4 in one engine call
// (cls_reach_external): the engine evaluates one representative address per
// address class of the bound ACLs, through the node's output interface, and
// returns only the maximal ranges, in (direction, Probe, Pod, Lo) order with
// egress first, the ranges of one (direction, probe, pod) covering
// 0..0xFFFFFFFF.  egress, ingress: the directions wanted.  Pods that
// ConnectionPodToInternet / ConnectionInternetToPod fail before
// testConnection (unregistered, on another node, without an interface, or an
// empty node output interface name) stay out of the call: each has the one
// range 0..0xFFFFFFFF of ConnActionFailure.
func (en *Engine) ReachExternal(pods []podmodel.ID, probes []Probe, egress, ingress bool) ([]AddrRange, error) {
	en.Lock()
	defer en.Unlock()
	N, P := len(pods), len(probes)
	var dirs []bool // Ingress of each direction index
	var mask uint32
	if egress {
		dirs, mask = append(dirs, false), mask|1
	}
	if ingress {
		dirs, mask = append(dirs, true), mask|2
	}
	if P == 0 || len(dirs) == 0 {
		return nil, nil
	}
	var strs cstrs
	defer strs.free()
	extName := en.nodeOutputIf()
	var at []int // endpoint -> index in pods
	var ifs []uint32
	var ips []net.IP
	inside := make([]int, N) // 1 + the pod's endpoint, 0: left out
	v4 := true
	for i, pod := range pods {
		cfg := en.pods[pod]
		if cfg == nil || cfg.anotherNode || extName == "" {
			continue
		}
		ifName, ok := en.Contiv.GetIfName(pod.Namespace, pod.Name)
		if !ok {
			continue
		}
		var v C.uint32_t
		C.cls_if_id(en.e, strs.add(ifName), &v)
		at, ifs, ips = append(at, i), append(ifs, uint32(v)), append(ips, cfg.ip)
		inside[i] = len(at)
		v4 = v4 && cfg.ip.To4() != nil
	}
	n := len(at)
	var rec []uint32 // 16-byte records: src, probe | dir << 16 | action << 24, lo, hi
	total := 0
	if n > 0 {
		var ext C.uint32_t
		C.cls_if_id(en.e, strs.add(extName), &ext)
		a4 := make([]uint32, n)
		a16 := make([]byte, 16*n)
		for k := 0; k < n; k++ {
			if v4 {
				a := ips[k].To4()
				a4[k] = uint32(a[0])<<24 | uint32(a[1])<<16 | uint32(a[2])<<8 | uint32(a[3])
			} else {
				a := ips[k].To16()
				if a == nil {
					return nil, errors.New("connection endpoint is not an IPv4 or IPv6 address")
				}
				copy(a16[16*k:], a)
			}
		}
		pr, sp, dp := make([]uint8, P), make([]uint16, P), make([]uint16, P)
		for k, q := range probes {
			pr[k], sp[k], dp[k] = uint8(q.Protocol), q.SrcPort, q.DstPort
		}
		// every slice goes to the shim as its own pointer (pointer-free Go
		// memory); the shim builds both structs on the C stack.  The ranges
		// are counted first, then fetched.
		var count C.uint64_t
		for pass := 0; pass < 2; pass++ {
			var buf unsafe.Pointer
			if pass == 1 {
				rec = make([]uint32, 4*int(count))
				buf = unsafe.Pointer(&rec[0])
			}
			var rc C.int
			if v4 {
				rc = C.clsg_reach_external_v4(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint32_t)(&a4[0]), C.uint32_t(n),
					(*C.uint8_t)(&pr[0]), (*C.uint16_t)(&sp[0]), (*C.uint16_t)(&dp[0]), C.uint32_t(P), ext,
					C.uint32_t(mask), buf, count, &count, nil, nil, nil, nil, 0)
			} else {
				rc = C.clsg_reach_external_v16(en.e, (*C.uint32_t)(&ifs[0]), (*C.uint8_t)(&a16[0]), C.uint32_t(n),
					(*C.uint8_t)(&pr[0]), (*C.uint16_t)(&sp[0]), (*C.uint16_t)(&dp[0]), C.uint32_t(P), ext,
					C.uint32_t(mask), buf, count, &count, nil, nil, nil, nil, 0)
			}
			if rc != C.CLS_OK {
				return nil, en.lastErr()
			}
		}
		total = len(rec) / 4
		if int(count) < total { // (the bindings cannot change under the lock)
			total = int(count)
		}
	}
	// merge, in line order, with the lines of the pods left out (at is
	// ascending, so the engine's records are in line order over pods too)
	var out []AddrRange
	k := 0
	for _, in := range dirs {
		for p := 0; p < P; p++ {
			for s := 0; s < N; s++ {
				if inside[s] == 0 {
					out = append(out, AddrRange{Ingress: in, Probe: p, Pod: s, Lo: 0, Hi: 0xFFFFFFFF,
						Action: aclengine.ConnActionFailure})
					continue
				}
				for k < total && int(rec[4*k]) == inside[s]-1 && int(rec[4*k+1]&0xFFFF) == p &&
					(rec[4*k+1]>>16&0xFF != 0) == in {
					out = append(out, AddrRange{Ingress: in, Probe: p, Pod: s, Lo: rec[4*k+2], Hi: rec[4*k+3],
						Action: aclengine.ConnectionAction(rec[4*k+1] >> 24)})
					k++
				}
			}
		}
	}
	return out, nil
}

// Table is one compiled ACL on the device (cls_table_put), for batched
// classification outside the renderer's bindings.
type Table struct {
	ID     uint32
	NRules int
}

// PutTable compiles and uploads an ACL's rules (evalACL semantics).
func (en *Engine) PutTable(acl *vpp_acl.AccessLists_Acl) (*Table, error) {
	en.Lock()
	defer en.Unlock()
	var strs cstrs
	defer strs.free()
	rules := flatten(acl, &strs)
	var rp *C.cls_rule
	if len(rules) > 0 {
		rp = &rules[0]
	}
	var id C.uint32_t
	if rc := C.cls_table_put(en.e, strs.add(acl.AclName), rp, C.uint32_t(len(rules)), &id); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	return &Table{ID: uint32(id), NRules: len(rules)}, nil
}

// DelTable frees a table (its pending device work finishes first).
func (en *Engine) DelTable(t *Table) error {
	en.Lock()
	defer en.Unlock()
	if rc := C.cls_table_del(en.e, C.uint32_t(t.ID)); rc != C.CLS_OK {
		return en.lastErr()
	}
	return nil
}

// ClassifyBatch: evalACL (aclengine_mock.go:473-668) for every packet of an
// IPv4 batch (host-order addresses), and the per-rule hit counters
// (counters[k], k < R: packets that terminated at rule k; counters[R]: the
// default DENY).
func (en *Engine) ClassifyBatch(t *Table, src, dst []uint32, dport []uint16,
	proto []aclengine.ProtocolType) ([]uint8, []uint64, error) {
	n := len(src)
	if len(dst) != n || len(dport) != n || len(proto) != n {
		return nil, nil, errors.New("contivcls: packet arrays of different lengths")
	}
	verdict := make([]uint8, n)
	counters := make([]uint64, t.NRules+1)
	if n == 0 {
		return verdict, counters, nil
	}
	pr := make([]uint8, n)
	for i, p := range proto {
		pr[i] = uint8(p)
	}
	en.Lock()
	defer en.Unlock()
	if rc := C.clsg_classify_v4(en.e, C.uint32_t(t.ID), (*C.uint32_t)(&src[0]), (*C.uint32_t)(&dst[0]),
		(*C.uint16_t)(&dport[0]), (*C.uint8_t)(&pr[0]), C.uint64_t(n), (*C.uint8_t)(&verdict[0]),
		(*C.uint64_t)(&counters[0]), 0); rc != C.CLS_OK {
		return nil, nil, en.lastErr()
	}
	return verdict, counters, nil
}

// ClassifyBatchRules: each packet's ACLAction and the index of the rule at
// which evalACL terminated (t.NRules: the default DENY) -- the matched rule
// evalACL logs at Debug (aclengine_mock.go:651-654), for a whole batch; no
// counters.
func (en *Engine) ClassifyBatchRules(t *Table, src, dst []uint32, dport []uint16,
	proto []aclengine.ProtocolType) ([]uint8, []uint32, error) {
	n := len(src)
	if len(dst) != n || len(dport) != n || len(proto) != n {
		return nil, nil, errors.New("contivcls: packet arrays of different lengths")
	}
	verdict := make([]uint8, n)
	rules := make([]uint32, n)
	if n == 0 {
		return verdict, rules, nil
	}
	pr := make([]uint8, n)
	for i, p := range proto {
		pr[i] = uint8(p)
	}
	en.Lock()
	defer en.Unlock()
	if rc := C.clsg_classify_rules_v4(en.e, C.uint32_t(t.ID), (*C.uint32_t)(&src[0]), (*C.uint32_t)(&dst[0]),
		(*C.uint16_t)(&dport[0]), (*C.uint8_t)(&pr[0]), C.uint64_t(n), (*C.uint8_t)(&verdict[0]),
		(*C.uint32_t)(&rules[0])); rc != C.CLS_OK {
		return nil, nil, en.lastErr()
	}
	return verdict, rules, nil
}

// ClassifyBatchIP: the same for addresses of any family (net.IP; IPv4 and
// IPv4-mapped packets match IPv4 networks only, as Go's IPNet.Contains).
func (en *Engine) ClassifyBatchIP(t *Table, src, dst []net.IP, dport []uint16,
	proto []aclengine.ProtocolType) ([]uint8, []uint64, error) {
	n := len(src)
	if len(dst) != n || len(dport) != n || len(proto) != n {
		return nil, nil, errors.New("contivcls: packet arrays of different lengths")
	}
	verdict := make([]uint8, n)
	counters := make([]uint64, t.NRules+1)
	if n == 0 {
		return verdict, counters, nil
	}
	s16, d16, pr := make([]byte, 16*n), make([]byte, 16*n), make([]uint8, n)
	for i := 0; i < n; i++ {
		a, b := src[i].To16(), dst[i].To16()
		if a == nil || b == nil {
			return nil, nil, errors.New("contivcls: packet address is not an IPv4 or IPv6 address")
		}
		copy(s16[16*i:], a)
		copy(d16[16*i:], b)
		pr[i] = uint8(proto[i])
	}
	en.Lock()
	defer en.Unlock()
	if rc := C.clsg_classify_v16(en.e, C.uint32_t(t.ID), (*C.uint8_t)(&s16[0]), (*C.uint8_t)(&d16[0]),
		(*C.uint16_t)(&dport[0]), (*C.uint8_t)(&pr[0]), C.uint64_t(n), (*C.uint8_t)(&verdict[0]),
		(*C.uint64_t)(&counters[0]), 0); rc != C.CLS_OK {
		return nil, nil, en.lastErr()
	}
	return verdict, counters, nil
}

// ConnCounters: the per-(ACL, rule) hit counters of the connection path for
// the installed ACL aclName (cls_conn_counters; reset clears them).
func (en *Engine) ConnCounters(aclName string, reset bool) ([]uint64, error) {
	en.Lock()
	defer en.Unlock()
	var strs cstrs
	defer strs.free()
	var id C.uint32_t
	if rc := C.cls_acl_table(en.e, strs.add(aclName), &id); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	var info C.cls_table_info
	if rc := C.cls_table_get_info(en.e, id, &info); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	out := make([]uint64, int(info.n_rules)+1)
	r := C.uint32_t(0)
	if reset {
		r = 1
	}
	if rc := C.cls_conn_counters(en.e, id, (*C.uint64_t)(&out[0]), r); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	return out, nil
}

// Witness is the least packet, in (Src, Dst, Protocol, DstPort) order, that
// terminates at a rule: addresses in host order, Protocol 0 TCP, 1 UDP, 2 ICMP
// and 3 standing for every other value.
type Witness struct {
	Src, Dst uint32
	Protocol uint8
	DstPort  uint16
}

// Coverage is TableCover's answer for one installed ACL: Dead, the indices of
// the rules no IPv4 packet can terminate at; Witnesses, rule index -> a packet
// that terminates there; DefaultReachable, whether some packet falls through
// to the default DENY; Cells, the cells of the class product the engine swept.
type Coverage struct {
	Dead             []int
	Witnesses        map[int]Witness
	DefaultReachable bool
	Cells            uint64
}

// TableCover answers "which rules of this ACL can never be the matched rule,
// and which packet matches each of the others?" in one engine call
// (cls_table_cover): the engine sweeps every cell of source class x
// destination class x (protocol, port class) of the ACL's compiled table on
// the device.  The sweep covers the IPv4 packet space: a rule that only native
// IPv6 packets can reach is reported dead.  The reference has no counterpart;
// the closest is the matched rule evalACL logs at Debug.
func (en *Engine) TableCover(aclName string) (*Coverage, error) {
	en.Lock()
	defer en.Unlock()
	var strs cstrs
	defer strs.free()
	var id C.uint32_t
	if rc := C.cls_acl_table(en.e, strs.add(aclName), &id); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	var info C.cls_table_info
	if rc := C.cls_table_get_info(en.e, id, &info); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	r := int(info.n_rules)
	live := make([]uint8, r+1)
	rec := make([]uint32, 4*(r+1)) // 16-byte records: src, dst, dport | proto << 16 | live << 24, 0
	var cells C.uint64_t
	// every slice goes to the shim as its own pointer (pointer-free Go
	// memory); the shim builds the struct on the C stack
	if rc := C.clsg_table_cover_v4(en.e, id, (*C.uint8_t)(&live[0]), unsafe.Pointer(&rec[0]), nil, nil, &cells, nil,
		0); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	out := &Coverage{Witnesses: make(map[int]Witness), DefaultReachable: live[r] != 0, Cells: uint64(cells)}
	for k := 0; k < r; k++ {
		if live[k] == 0 {
			out.Dead = append(out.Dead, k)
			continue
		}
		out.Witnesses[k] = Witness{Src: rec[4*k], Dst: rec[4*k+1], Protocol: uint8(rec[4*k+2] >> 16),
			DstPort: uint16(rec[4*k+2])}
	}
	return out, nil
}

// NeededBy is why TableNeed calls a rule needed: the least packet whose
// ACLAction changes once the rule is deleted, the action it then gets (After)
// and the rule that then takes it (Fall; the rule count: the default DENY).
type NeededBy struct {
	Packet Witness
	After  uint8
	Fall   int
}

// Need is TableNeed's answer for one installed ACL: Dead, the rules no IPv4
// packet terminates at; Redundant, the live rules whose packets all get the
// same ACLAction from the rest of the list once the rule alone is gone; Free,
// the dead and redundant rules that can be deleted together without changing
// a verdict (redundant rules are not jointly removable in general); Needed,
// rule index -> why; DefaultReachable; Cells, the cells the engine swept.
type Need struct {
	Dead, Redundant, Free []int
	Needed                map[int]NeededBy
	DefaultReachable      bool
	Cells                 uint64
}

// TableNeed answers "which rules does this ACL actually need?" in one engine
// call (cls_table_need) with the rules skip treated as deleted.  The sweep
// covers the IPv4 packet space: a rule with an IPv6 network is reported dead.
// The reference has no counterpart.
func (en *Engine) TableNeed(aclName string, skip []int) (*Need, error) {
	en.Lock()
	defer en.Unlock()
	var strs cstrs
	defer strs.free()
	var id C.uint32_t
	if rc := C.cls_acl_table(en.e, strs.add(aclName), &id); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	var info C.cls_table_info
	if rc := C.cls_table_get_info(en.e, id, &info); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	r := int(info.n_rules)
	mask := make([]uint64, (r+63)/64+1)
	for _, k := range skip {
		if k < 0 || k >= r {
			return nil, fmt.Errorf("contivcls: TableNeed: skip names rule %d of %d", k, r)
		}
		mask[k>>6] |= 1 << uint(k&63)
	}
	need := make([]uint8, r+1)
	free := make([]uint8, r+1)
	first := make([]uint64, r+1)
	rec := make([]uint32, 4*(r+1)) // 16-byte records: src, dst, dport | proto << 16 | after << 24, fall
	var cells C.uint64_t
	// every slice goes to the shim as its own pointer (pointer-free Go
	// memory); the shim builds the struct on the C stack
	if rc := C.clsg_table_need(en.e, id, (*C.uint64_t)(&mask[0]), (*C.uint8_t)(&need[0]), (*C.uint8_t)(&free[0]),
		(*C.uint64_t)(&first[0]), nil, unsafe.Pointer(&rec[0]), nil, &cells, nil, 0); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	out := &Need{Needed: make(map[int]NeededBy), DefaultReachable: first[r] != 0, Cells: uint64(cells)}
	for k := 0; k < r; k++ {
		switch need[k] {
		case C.CLS_NEED_DEAD:
			out.Dead = append(out.Dead, k)
		case C.CLS_NEED_REDUNDANT:
			out.Redundant = append(out.Redundant, k)
		case C.CLS_NEED_NEEDED:
			out.Needed[k] = NeededBy{Packet: Witness{Src: rec[4*k], Dst: rec[4*k+1], Protocol: uint8(rec[4*k+2] >> 16),
				DstPort: uint16(rec[4*k+2])}, After: uint8(rec[4*k+2]>>24) & 3, Fall: int(rec[4*k+3])}
		}
		if free[k] != 0 {
			out.Free = append(out.Free, k)
		}
	}
	return out, nil
}

// DiffRecord is one run of packets whose ACLAction differs between two ACLs:
// source and destination address ranges (host order, inclusive), Protocol 0
// TCP, 1 UDP, 2 ICMP and 3 standing for every other value, the destination
// port range (0 .. 65535 where the protocol has no port), the action under
// the first ACL (Was) and under the second (Now), and the rule each one's
// evaluation terminated at (the rule count: the default DENY).
type DiffRecord struct {
	SrcLo, SrcHi, DstLo, DstHi uint32
	PortLo, PortHi             uint16
	Protocol, Was, Now         uint8
	RuleA, RuleB               int
}

// Diff is TableDiff's answer for two installed ACLs: Equal, whether every IPv4
// packet gets the same ACLAction under both; Pairs[was][now], the cells of the
// joint class product per pair of actions; First, the least differing packet
// (nil if none); Records, the differing packets in ascending order; RulesA and
// RulesB, rule index -> the least differing packet that terminates there.
type Diff struct {
	Equal   bool
	Cells   uint64
	Pairs   [4][4]uint64
	First   *Witness
	Records []DiffRecord
	RulesA  map[int]Witness
	RulesB  map[int]Witness
}

func diffWitnesses(rec []uint32, r int) map[int]Witness {
	out := make(map[int]Witness)
	for k := 0; k <= r; k++ {
		if rec[4*k+2]>>24 == 0 {
			continue
		}
		out[k] = Witness{Src: rec[4*k], Dst: rec[4*k+1], Protocol: uint8(rec[4*k+2] >> 16), DstPort: uint16(rec[4*k+2])}
	}
	return out
}

// TableDiff answers "is ACL b semantically the same as ACL a, and if not, for
// exactly which packets does the verdict change, and which rules are
// responsible?" (cls_table_diff): the engine evaluates every cell of the two
// compiled tables' joint classes under both on the device and compares there.
// Two calls: the first counts the records, the second takes them.  The diff
// covers the IPv4 packet space.  The reference has no counterpart.
func (en *Engine) TableDiff(aclA, aclB string) (*Diff, error) {
	en.Lock()
	defer en.Unlock()
	var strs cstrs
	defer strs.free()
	var ids [2]C.uint32_t
	var rules [2]int
	for i, name := range []string{aclA, aclB} {
		if rc := C.cls_acl_table(en.e, strs.add(name), &ids[i]); rc != C.CLS_OK {
			return nil, en.lastErr()
		}
		var info C.cls_table_info
		if rc := C.cls_table_get_info(en.e, ids[i], &info); rc != C.CLS_OK {
			return nil, en.lastErr()
		}
		rules[i] = int(info.n_rules)
	}
	var nRec, nDiff, cells C.uint64_t
	if rc := C.clsg_table_diff_v4(en.e, ids[0], ids[1], nil, nil, nil, nil, nil, nil, nil, nil, 0, &nRec, nil, nil,
		0); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	// every slice goes to the shim as its own pointer (pointer-free Go
	// memory); the shim builds the struct on the C stack
	pairs := make([]uint64, 16)
	first := make([]uint32, 4)
	witA := make([]uint32, 4*(rules[0]+1)) // 16-byte records: src, dst, dport | proto << 16 | live << 24, 0
	witB := make([]uint32, 4*(rules[1]+1))
	rec := make([]uint32, 8*(int(nRec)+1)) // 32-byte records
	if rc := C.clsg_table_diff_v4(en.e, ids[0], ids[1], &nDiff, (*C.uint64_t)(&pairs[0]), unsafe.Pointer(&first[0]),
		nil, unsafe.Pointer(&witA[0]), nil, unsafe.Pointer(&witB[0]), unsafe.Pointer(&rec[0]), nRec, &nRec, &cells,
		nil, 0); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	out := &Diff{Equal: nDiff == 0, Cells: uint64(cells), RulesA: diffWitnesses(witA, rules[0]),
		RulesB: diffWitnesses(witB, rules[1])}
	for i := 0; i < 16; i++ {
		out.Pairs[i/4][i%4] = pairs[i]
	}
	if first[2]>>24 != 0 {
		out.First = &Witness{Src: first[0], Dst: first[1], Protocol: uint8(first[2] >> 16), DstPort: uint16(first[2])}
	}
	for k := 0; k < int(nRec) && 8*k+7 < len(rec); k++ {
		w := rec[8*k : 8*k+8]
		out.Records = append(out.Records, DiffRecord{SrcLo: w[0], SrcHi: w[1], DstLo: w[2], DstHi: w[3],
			PortLo: uint16(w[4]), PortHi: uint16(w[4] >> 16), Protocol: uint8(w[5]), Was: uint8(w[5] >> 8),
			Now: uint8(w[5] >> 16), RuleA: int(w[6]), RuleB: int(w[7])})
	}
	return out, nil
}

// ---- HBM-resident batches (ABI 4) -------------------------------------------
// A Batch is engine-owned memory: packets stay in HBM between calls and no
// Go pointer is ever kept by the library (cgo rule).  With mirror the batch
// also owns pinned host arrays (Mirror*) that Go fills in place; Upload(f,
// nil) then moves them at DMA speed.

// Batch fields (CLS_BF_*).
const (
	FieldSrc     = uint32(C.CLS_BF_SRC)
	FieldDst     = uint32(C.CLS_BF_DST)
	FieldSport   = uint32(C.CLS_BF_SPORT)
	FieldDport   = uint32(C.CLS_BF_DPORT)
	FieldProto   = uint32(C.CLS_BF_PROTO)
	FieldVerdict = uint32(C.CLS_BF_VERDICT)
	FieldSrcIf   = uint32(C.CLS_BF_SRC_IF)
	FieldDstIf   = uint32(C.CLS_BF_DST_IF)
)

type Batch struct {
	en *Engine
	b  *C.cls_batch
	N  int
	V6 bool
}

// NewBatch: n IPv4 (v6 false: host-order u32 addresses) or 16-byte packets;
// conn adds interface ids (ConnectBatchDevice).
func (en *Engine) NewBatch(n int, v6, conn, mirror bool) (*Batch, error) {
	en.Lock()
	defer en.Unlock()
	af := C.uint32_t(C.CLS_AF_V4)
	if v6 {
		af = C.CLS_AF_V16
	}
	fl := C.uint32_t(0)
	if conn {
		fl |= C.CLS_BATCH_CONN
	}
	if mirror {
		fl |= C.CLS_BATCH_MIRROR
	}
	var b *C.cls_batch
	if rc := C.cls_batch_create(en.e, af, C.uint64_t(n), fl, &b); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	return &Batch{en: en, b: b, N: n, V6: v6}, nil
}

// Close frees the batch (before its engine).
func (b *Batch) Close() {
	if b.b != nil {
		C.cls_batch_destroy(b.b)
		b.b = nil
	}
}

// MirrorU32 / MirrorU16 / MirrorU8: the pinned host array of a field (C
// memory: Go may keep and fill these slices), nil without CLS_BATCH_MIRROR.
// Go 1.9 slices C memory through a large array type (no unsafe.Slice).
func (b *Batch) MirrorU32(f uint32) []uint32 {
	p := C.clsg_batch_mirror(b.b, C.uint32_t(f))
	if p == nil {
		return nil
	}
	return (*[1 << 32]uint32)(p)[:b.N:b.N]
}
func (b *Batch) MirrorU16(f uint32) []uint16 {
	p := C.clsg_batch_mirror(b.b, C.uint32_t(f))
	if p == nil {
		return nil
	}
	return (*[1 << 33]uint16)(p)[:b.N:b.N]
}
func (b *Batch) MirrorU8(f uint32) []uint8 {
	p := C.clsg_batch_mirror(b.b, C.uint32_t(f))
	if p == nil {
		return nil
	}
	return (*[1 << 34]uint8)(p)[:b.N:b.N]
}

// Upload packets [first, first+n) of a field from src (the base of a Go
// slice of the field's element type: pointer-free Go memory, valid for the
// call), or from the mirror (src nil).
func (b *Batch) Upload(f uint32, first, n int, src unsafe.Pointer) error {
	if rc := C.cls_batch_upload(b.b, C.uint32_t(f), C.uint64_t(first), C.uint64_t(n), src); rc != C.CLS_OK {
		return b.en.lastErr()
	}
	return nil
}

// Verdicts of packets [first, first+n) (waits for the batch's work).
func (b *Batch) Verdicts(first, n int) ([]uint8, error) {
	out := make([]uint8, n)
	if n == 0 {
		return out, nil
	}
	if rc := C.cls_batch_download(b.b, C.CLS_BF_VERDICT, C.uint64_t(first), C.uint64_t(n),
		unsafe.Pointer(&out[0])); rc != C.CLS_OK {
		return nil, b.en.lastErr()
	}
	return out, nil
}

// ClassifyBatchDevice: evalACL over the whole batch on its devices; the hit
// counters summed over the shards (and over processes, CommInit).  wait
// false only enqueues (Counters reads the last call's).
func (en *Engine) ClassifyBatchDevice(t *Table, b *Batch, wait bool) ([]uint64, error) {
	var out []uint64
	var op *C.uint64_t
	if wait {
		out = make([]uint64, t.NRules+1)
		op = (*C.uint64_t)(&out[0])
	}
	if rc := C.cls_classify_batch(en.e, C.uint32_t(t.ID), b.b, op, 0); rc != C.CLS_OK {
		return nil, en.lastErr()
	}
	return out, nil
}

// Counters of the batch's last ClassifyBatchDevice.
func (b *Batch) Counters(t *Table) ([]uint64, error) {
	out := make([]uint64, t.NRules+1)
	if rc := C.cls_batch_counters(b.b, (*C.uint64_t)(&out[0]), C.uint32_t(len(out))); rc != C.CLS_OK {
		return nil, b.en.lastErr()
	}
	return out, nil
}

// ConnectBatchDevice: testConnection over a conn batch (ConnectionAction per
// connection into FieldVerdict).
func (en *Engine) ConnectBatchDevice(b *Batch, count bool) error {
	fl := C.uint32_t(0)
	if count {
		fl |= C.CLS_F_COUNT
	}
	if rc := C.cls_batch_connect(en.e, b.b, fl); rc != C.CLS_OK {
		return en.lastErr()
	}
	return nil
}

// CommUniqueID / CommInit: one process per GPU (or GPU group) joins one RCCL
// communicator for the counter merge; process 0 makes the id, the others get
// it out of band.
func CommUniqueID() ([128]byte, error) {
	var id [128]byte
	if rc := C.cls_comm_unique_id(unsafe.Pointer(&id[0])); rc != C.CLS_OK {
		return id, errors.New("contivcls: RCCL unavailable")
	}
	return id, nil
}

func (en *Engine) CommInit(nProcs, proc int, id *[128]byte) error {
	var p unsafe.Pointer
	if id != nil {
		p = C.CBytes(id[:])
		defer C.free(p)
	}
	if rc := C.cls_comm_init(en.e, C.uint32_t(nProcs), C.uint32_t(proc), p); rc != C.CLS_OK {
		return en.lastErr()
	}
	return nil
}
