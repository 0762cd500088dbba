//go:build swp

// Package scheduler — cgo binding of libswp.so behind manager/scheduler.Scheduler.
//
// Drop this file next to manager/scheduler/nodeset.go and build with `-tags swp` (CGO_ENABLED=1, third_party/swp/{include,lib}
// holding include/swp.h and libswp.so of this repository). It mirrors every nodeSet / NodeInfo mutator into the engine and
// replaces the two branches of tick() (scheduler.go:456-469) with swp_schedule_groups / swp_schedule_batch; everything
// else of the reference — event handlers, store commits, noSuitableNode — stays as it is. Tasks the engine declines
// (more than 32 host ports, more than 8 generic kinds or cluster mounts, Named generic reservations) keep running through the
// reference's scheduleTaskGroup. CSI cluster volumes ARE on the engine: volumeSet keeps its maps, the hooks below mirror them
// (upsertVolume from addOrUpdateVolume, pushVolumeUsage from reserveVolume / releaseVolume, nodeCSI with every node row), the batch
// returns the attachments chooseTaskVolumes would have picked and the caller runs its own reserveTaskVolumes on them.
//
// A manager on a multi-GPU box holds a shard SET instead of an engine (newSwpShardSet: swp_shardset_create): the same handle type,
// the same calls — the set routes node calls to the owner of the node's range and runs a batch over all ranges.
//
// NOT COMPILED IN THIS REPOSITORY: the build image has no Go toolchain. The same layer, with the same function names and
// the reference's line numbers, is implemented and tested in C++ (swarmkit_amd/csrc/swp_sched.cpp, include/swp_sched.h);
// every helper below is the Go spelling of the C++ method named in its comment.
package scheduler

/*
#cgo CFLAGS: -I${SRCDIR}/../../third_party/swp/include
#cgo LDFLAGS: -L${SRCDIR}/../../third_party/swp/lib -lswp
#include <stdlib.h>
#include "swp.h"
*/
import "C"

import (
	"context"
	"fmt"
	"net"
	"runtime/cgo"
	"sort"
	"strconv"
	"strings"
	"time"
	"unsafe"

	"github.com/moby/swarmkit/v2/api"
	"github.com/moby/swarmkit/v2/api/genericresource"
	"github.com/moby/swarmkit/v2/manager/constraint"
)

type swpEngine struct {
	e       *C.swp_engine
	idxNode []string // dense node index (a removed node's index goes to the next new node: entries are overwritten) -> api.Node.ID
	nodeIdx map[string]C.uint32_t // the inverse, for volume usage (dropped on nodeSet.remove)
	volumeID []string             // SWP_SPACE_VOLUME index -> api.Volume.ID
	vs      *volumeSet            // Scheduler.volumes: byName resolves a mount's Source when the task's descriptor is built
	// failure counts the engine holds: a bucket erased by cleanupFailures must be reset there too (Scheduler::pushFailures)
	pushed map[failureBucket]uint32
	// generic kinds a node's available list holds in a way one count per kind cannot stand for (irregularKinds below), per node index:
	// a task that reserves such a kind keeps running through the reference's path (genericSet)
	irregular map[C.uint32_t]map[string]bool
}

type failureBucket struct {
	node    C.uint32_t
	service string
	version uint64
}

// vs: the scheduler's volumeSet (Scheduler.volumes): mountSet resolves a mount's Source through vs.byName
func newSwpEngine(device int, vs *volumeSet) (*swpEngine, error) {
	cfg := C.swp_config{device: C.int32_t(device)}
	var e *C.swp_engine
	if rc := C.swp_create(&cfg, &e); rc != C.SWP_OK {
		return nil, fmt.Errorf("swp_create: %s", C.GoString(C.swp_last_error(nil))) // SWP_ENODEVICE: keep the Go path
	}
	return &swpEngine{e: e, vs: vs, nodeIdx: map[string]C.uint32_t{}, pushed: map[failureBucket]uint32{}, irregular: map[C.uint32_t]map[string]bool{}}, nil
}

// newSwpShardSet: one engine per GPU of the box behind ONE handle (swp_shardset_create, include/swp.h "A shard SET"): node i of the
// canonical order lives on engine i / nodesPerShard. Everything below is the same for a set and for an engine.
func newSwpShardSet(devices []int, nodesPerShard int, vs *volumeSet) (*swpEngine, error) {
	cfg := C.swp_config{device: C.int32_t(devices[0])}
	devs := make([]C.int32_t, len(devices))
	for i, d := range devices {
		devs[i] = C.int32_t(d)
	}
	var e *C.swp_engine
	if rc := C.swp_shardset_create(&cfg, &devs[0], C.uint32_t(len(devs)), C.uint32_t(nodesPerShard), &e); rc != C.SWP_OK {
		return nil, fmt.Errorf("swp_shardset_create: %s", C.GoString(C.swp_last_error(nil)))
	}
	return &swpEngine{e: e, vs: vs, nodeIdx: map[string]C.uint32_t{}, pushed: map[failureBucket]uint32{}}, nil
}

func (s *swpEngine) close() { C.swp_destroy(s.e) }

func (s *swpEngine) err(what string, rc C.int) error {
	return fmt.Errorf("%s: %s: %s", what, C.GoString(C.swp_strerror(rc)), C.GoString(C.swp_last_error(s.e)))
}

// Scheduler::intern
func (s *swpEngine) intern(space C.int, v string) C.uint32_t {
	var id C.uint32_t
	var p *C.char
	if len(v) > 0 {
		p = (*C.char)(unsafe.Pointer(unsafe.StringData(v))) // read during the call only; not retained (cgo pointer rules)
	}
	C.swp_intern(s.e, space, p, C.size_t(len(v)), &id)
	return id
}

func (s *swpEngine) folded(v string) C.uint32_t { return s.intern(C.SWP_SPACE_FOLDED, v) }

func (s *swpEngine) nodeIndex(id string) C.uint32_t {
	idx := s.intern(C.SWP_SPACE_NODE_ID, id)
	for len(s.idxNode) <= int(idx) {
		s.idxNode = append(s.idxNode, "")
	}
	s.idxNode[idx] = id
	s.nodeIdx[id] = idx
	return idx
}

// ---------------------------------------------------------------------------------------------- nodeSet mirror

// parseIP16: net.ParseIP as the 16-byte form the engine compares (v4 as ::ffff:a.b.c.d); Scheduler::parse_ip
func parseIP16(addr string) (ip [16]C.uint8_t, ok, v4 bool) {
	p := net.ParseIP(addr)
	if p == nil {
		return ip, false, false
	}
	p16 := p.To16()
	for i := 0; i < 16; i++ {
		ip[i] = C.uint8_t(p16[i])
	}
	return ip, true, p.To4() != nil
}

func (s *swpEngine) kvs(labels map[string]string) []C.swp_kv {
	keys := make([]string, 0, len(labels))
	for k := range labels {
		keys = append(keys, k)
	}
	sort.Strings(keys) // any order: the engine stores a set
	out := make([]C.swp_kv, 0, len(keys))
	for _, k := range keys {
		out = append(out, C.swp_kv{key: s.intern(C.SWP_SPACE_LABEL_KEY, k), value: s.folded(labels[k]), raw: s.intern(C.SWP_SPACE_RAW, labels[k])})
	}
	return out
}

// upsert: nodeSet.addOrUpdateNode / updateNode (nodeset.go:33-44) wherever the Go code stores a NodeInfo; Scheduler::upsertRow
func (s *swpEngine) upsert(n NodeInfo) error {
	row := C.swp_node_row{
		node:    s.nodeIndex(n.ID),
		cpu:     C.int64_t(n.AvailableResources.NanoCPUs),
		mem:     C.int64_t(n.AvailableResources.MemoryBytes),
		total:   C.uint32_t(n.ActiveTasksCount),
		id_fold: s.folded(n.ID),
		version: C.uint64_t(n.Meta.Version.Index),
	}
	var flags C.uint32_t
	if n.Status.State == api.NodeStatus_READY && n.Spec.Availability == api.NodeAvailabilityActive { // ReadyFilter, filter.go:41-44
		flags |= C.SWP_NODE_READY
	}
	if n.Role == api.NodeRoleManager {
		flags |= C.SWP_NODE_MANAGER
	}
	var lab, elab []C.swp_kv
	var plugins []C.uint32_t
	if n.Spec.Annotations.Labels != nil {
		flags |= C.SWP_NODE_HAS_LABELS
		lab = s.kvs(n.Spec.Annotations.Labels)
	}
	if d := n.Description; d != nil {
		flags |= C.SWP_NODE_HAS_DESC
		row.hostname_fold = s.folded(d.Hostname)
		if p := d.Platform; p != nil {
			flags |= C.SWP_NODE_HAS_PLATFORM
			row.os = s.intern(C.SWP_SPACE_OS, p.OS)
			row.arch = s.intern(C.SWP_SPACE_ARCH, p.Architecture) // the engine normalises x86_64 / aarch64 (filter.go:285-299)
			row.os_fold = s.folded(p.OS)
			row.arch_fold = s.folded(p.Architecture)
		}
		if e := d.Engine; e != nil {
			flags |= C.SWP_NODE_HAS_ENGINE
			if e.Labels != nil {
				flags |= C.SWP_NODE_HAS_ELABELS
				elab = s.kvs(e.Labels)
			}
			for _, p := range e.Plugins {
				if p.Type == "Log" {
					flags |= C.SWP_NODE_HAS_LOGPLUG
				}
				plugins = append(plugins, s.intern(C.SWP_SPACE_PLUGIN, p.Type+"\x00"+p.Name))
				if strings.HasSuffix(p.Name, ":latest") { // filter.go:189-199: "name" also matches "name:latest"
					plugins = append(plugins, s.intern(C.SWP_SPACE_PLUGIN, p.Type+"\x00"+strings.TrimSuffix(p.Name, ":latest")))
				}
			}
		}
	}
	if ip, ok, v4 := parseIP16(n.Status.Addr); ok {
		row.ip = ip
		flags |= C.SWP_NODE_IP_VALID
		if v4 {
			flags |= C.SWP_NODE_IP_V4
		}
	}
	row.flags = flags
	var noKV C.swp_kv
	var noPlugin C.uint32_t
	labP, elabP, plugP := &noKV, &noKV, &noPlugin
	if len(lab) > 0 {
		labP = &lab[0]
	}
	if len(elab) > 0 {
		elabP = &elab[0]
	}
	if len(plugins) > 0 {
		plugP = &plugins[0]
	}
	if rc := C.swp_node_upsert(s.e, &row, labP, C.uint32_t(len(lab)), elabP, C.uint32_t(len(elab)), plugP, C.uint32_t(len(plugins))); rc != C.SWP_OK {
		return s.err("swp_node_upsert", rc)
	}
	for svc, c := range n.ActiveTasksCountByService {
		C.swp_node_set_svc_count(s.e, row.node, s.intern(C.SWP_SPACE_SERVICE, svc), C.uint32_t(c))
	}
	for spec := range n.usedHostPorts {
		C.swp_node_port(s.e, row.node, C.uint32_t(spec.protocol), C.uint32_t(spec.publishedPort), 1)
	}
	if n.Description != nil {
		s.nodeCSI(row.node, n.Description.CSIInfo)
	} else {
		s.nodeCSI(row.node, nil)
	}
	return s.pushGeneric(row.node, n.AvailableResources.Generic)
}

// genericCounts: AvailableResources.Generic as ONE count per kind, as genericresource.HasEnough (validate.go:24-52) reads the list: the
// FIRST entry of the kind decides — a Discrete entry counts its Value, a Named one counts the Named entries of the kind (a list that
// mixes both for one kind, which sanitize can leave behind after a node changed its resource type, is judged by its first entry).
// Same rule as csrc/swp_generic.hpp counts().
func (s *swpEngine) genericCounts(rs []*api.GenericResource) []C.swp_generic {
	acc := map[string]int64{}
	discrete := map[string]bool{}
	var order []string
	for _, r := range rs {
		k := genericresource.Kind(r)
		d := r.GetDiscreteResourceSpec()
		if _, seen := acc[k]; !seen {
			order = append(order, k)
			discrete[k] = d != nil
			if d != nil {
				acc[k] = d.Value
			} else {
				acc[k] = 1
			}
			continue
		}
		if !discrete[k] && d == nil {
			acc[k]++ // another Named value of a kind whose first entry is Named
		}
	}
	out := make([]C.swp_generic, 0, len(order))
	for _, k := range order {
		if acc[k] > 0 {
			out = append(out, C.swp_generic{kind: s.intern(C.SWP_SPACE_GENERIC_KIND, k), value: C.int64_t(acc[k])})
		}
	}
	return out
}

// irregularKinds: the kinds of an available list ONE count cannot stand for — more than one entry of the kind and not all of them
// Named, or a Named value listed twice. Reclaim + sanitize (resource_management.go:75-153) leave such lists behind when a node's
// description changed under a running task and that task goes away. HasEnough reads the first entry (or counts the entries),
// ConsumeNodeResources (helpers.go:87-111) subtracts a claim from EVERY Discrete entry of the kind and removes EVERY entry with a claimed
// name: the engine's arithmetic inside a batch (count -= request) is then not the list's. csrc/swp_generic.hpp irregular_kinds();
// found by round 6's 20 000-seed soak (tests/test_engine_generic.py).
func irregularKinds(rs []*api.GenericResource) map[string]bool {
	entries, discrete := map[string]int{}, map[string]int{}
	names := map[[2]string]bool{}
	out := map[string]bool{}
	for _, r := range rs {
		k := genericresource.Kind(r)
		entries[k]++
		if r.GetDiscreteResourceSpec() != nil {
			discrete[k]++
		} else if n := r.GetNamedResourceSpec(); n != nil {
			if names[[2]string{k, n.Value}] {
				out[k] = true
			}
			names[[2]string{k, n.Value}] = true
		}
	}
	for k, n := range entries {
		if n > 1 && discrete[k] > 0 {
			out[k] = true
		}
	}
	return out
}

// pushGeneric: after createOrUpdateNode and after every NodeInfo.addTask / removeTask that claimed or reclaimed generic resources
// outside a device batch (nodeinfo.go:95-104, 134-137)
func (s *swpEngine) pushGeneric(node C.uint32_t, rs []*api.GenericResource) error {
	if irr := irregularKinds(rs); len(irr) > 0 {
		s.irregular[node] = irr
	} else {
		delete(s.irregular, node)
	}
	cnt := s.genericCounts(rs)
	var none C.swp_generic
	p := &none
	if len(cnt) > 0 {
		p = &cnt[0]
	}
	if rc := C.swp_node_set_generic(s.e, node, p, C.uint32_t(len(cnt))); rc != C.SWP_OK {
		return s.err("swp_node_set_generic", rc)
	}
	return nil
}

// genericSet: Reservations.Generic of a task (ResourceFilter.Check, filter.go:86-91). false: keep the task on the Go path.
func (s *swpEngine) genericSet(rs []*api.GenericResource) (C.uint32_t, bool) {
	if len(rs) == 0 {
		return 0, true
	}
	items := make([]C.swp_generic, 0, len(rs))
	for _, r := range rs {
		d := r.GetDiscreteResourceSpec() // a task reserves Discrete amounts (api/genericresource/parse.go); anything else stays in Go
		if d == nil || d.Value < 1 {
			return 0, false
		}
		for _, irr := range s.irregular { // some node lists this kind twice: the reference's own path decides the task (Scheduler::refuseIrregularGeneric)
			if irr[d.Kind] {
				return 0, false
			}
		}
		items = append(items, C.swp_generic{kind: s.intern(C.SWP_SPACE_GENERIC_KIND, d.Kind), value: C.int64_t(d.Value)})
	}
	var id C.uint32_t
	if rc := C.swp_generic_set(s.e, &items[0], C.uint32_t(len(items)), &id); rc != C.SWP_OK { // SWP_ERANGE (> 8 kinds), a kind twice
		return 0, false
	}
	return id, true
}

// remove: nodeSet.remove, nodeset.go:46-48. The index is LOOKED UP, never interned: interning an id the engine does not know would
// take an index out of the free pool for a node that is not there. The engine hands the index to the next new node: forget it here.
func (s *swpEngine) remove(nodeID string) {
	idx, ok := s.nodeIdx[nodeID]
	if !ok {
		return
	}
	C.swp_node_remove(s.e, idx)
	delete(s.irregular, idx)
	delete(s.nodeIdx, nodeID)
	s.idxNode[idx] = ""
	for b := range s.pushed { // failure buckets of the index that is free again
		if b.node == idx {
			delete(s.pushed, b)
		}
	}
	for id, info := range s.vs.volumes { // a volume in use on that node: none of the set's nodes is that node any more (Scheduler::repinVolumes)
		for _, usage := range info.tasks {
			if usage.nodeID == nodeID {
				s.pushVolumeUsage(id, info)
				break
			}
		}
	}
}

// drainBurst: a burst of availability flips (EventUpdateNode) in one call; Engine::node_update_dynamic_many
func (s *swpEngine) updateDynamic(rows []C.swp_node_dynamic) error {
	if len(rows) == 0 {
		return nil
	}
	if rc := C.swp_node_update_dynamic_many(s.e, &rows[0], C.uint32_t(len(rows))); rc != C.SWP_OK {
		return s.err("swp_node_update_dynamic_many", rc)
	}
	return nil
}

// ---------------------------------------------------------------------------------------------- Filter.SetTask helpers

// portSet: HostPortFilter.SetTask (filter.go:322-333); Scheduler::portSet
func (s *swpEngine) portSet(t *api.Task) (C.uint32_t, bool) {
	if t.Endpoint == nil {
		return 0, true
	}
	var ps []C.swp_port
	for _, p := range t.Endpoint.Ports {
		if p.PublishMode == api.PublishModeHost && p.PublishedPort != 0 {
			ps = append(ps, C.swp_port{protocol: C.uint32_t(p.Protocol), port: C.uint32_t(p.PublishedPort)})
		}
	}
	if len(ps) == 0 {
		return 0, true
	}
	if len(ps) > 32 {
		return 0, false // swp_port_set's limit: the task stays on the Go path
	}
	var id C.uint32_t
	if rc := C.swp_port_set(s.e, &ps[0], C.uint32_t(len(ps)), &id); rc != C.SWP_OK {
		return 0, false
	}
	return id, true
}

// labelKey: "node.labels.<name>" / "engine.labels.<name>" (prefix compared with EqualFold, the name is case-sensitive:
// constraint.go:177-199, nodeset.go:69-81); Scheduler::labelKey
func (s *swpEngine) labelKey(key string) (kind C.uint32_t, id C.uint32_t, ok bool) {
	const nl, el = "node.labels.", "engine.labels."
	if len(key) > len(nl) && strings.EqualFold(key[:len(nl)], nl) {
		return C.SWP_CK_NODE_LABEL, s.intern(C.SWP_SPACE_LABEL_KEY, key[len(nl):]), true
	}
	if len(key) > len(el) && strings.EqualFold(key[:len(el)], el) {
		return C.SWP_CK_ENGINE_LABEL, s.intern(C.SWP_SPACE_LABEL_KEY, key[len(el):]), true
	}
	return 0, 0, false
}

// constraintSet: ConstraintFilter.SetTask (filter.go:218-232) + the key dispatch of Constraint.Match (constraint.go:109-203);
// Scheduler::constraintStruct
func (s *swpEngine) constraintSet(cs []constraint.Constraint) C.uint32_t {
	if len(cs) == 0 {
		return 0
	}
	out := make([]C.swp_constraint, 0, len(cs))
	for _, x := range cs {
		c := C.swp_constraint{kind: C.SWP_CK_INVALID, op: C.uint32_t(x.Operator()), value: s.folded(x.Exp())} // accessors: add them to package constraint (key, operator, exp are unexported)
		key := x.Key()
		switch {
		case strings.EqualFold(key, "node.id"):
			c.kind = C.SWP_CK_NODE_ID
		case strings.EqualFold(key, "node.hostname"):
			c.kind = C.SWP_CK_HOSTNAME
		case strings.EqualFold(key, "node.ip"):
			c.kind = C.SWP_CK_IP
			c.ip_kind = C.SWP_IP_MALFORMED
			if ip, ok, v4 := parseIP16(x.Exp()); ok {
				c.ip, c.ip_kind = ip, C.SWP_IP_SINGLE
				if v4 {
					c.ip_is_v4 = 1
				}
			} else if _, subnet, err := net.ParseCIDR(x.Exp()); err == nil {
				ones, bits := subnet.Mask.Size()
				ip16 := subnet.IP.To16()
				for i := 0; i < 16; i++ {
					c.ip[i] = C.uint8_t(ip16[i])
				}
				c.ip_kind = C.SWP_IP_CIDR
				c.prefix_len = C.uint32_t(ones)
				if bits == 32 { // written as IPv4: the prefix counts in the 128-bit form
					c.prefix_len += 96
					c.ip_is_v4 = 1
				}
			}
		case strings.EqualFold(key, "node.role"):
			c.kind = C.SWP_CK_ROLE
		case strings.EqualFold(key, "node.platform.os"):
			c.kind = C.SWP_CK_PLATFORM_OS
		case strings.EqualFold(key, "node.platform.arch"):
			c.kind = C.SWP_CK_PLATFORM_ARCH
		default:
			if kind, id, ok := s.labelKey(key); ok {
				c.kind, c.key = kind, id
			}
		}
		out = append(out, c)
	}
	var id C.uint32_t
	C.swp_constraint_set(s.e, &out[0], C.uint32_t(len(out)), &id)
	return id
}

// platformSet: PlatformFilter.SetTask (filter.go:253-263)
func (s *swpEngine) platformSet(ps []*api.Platform) C.uint32_t {
	if len(ps) == 0 {
		return 0
	}
	out := make([]C.swp_platform, 0, len(ps))
	for _, p := range ps {
		out = append(out, C.swp_platform{os: s.intern(C.SWP_SPACE_OS, p.OS), arch: s.intern(C.SWP_SPACE_ARCH, p.Architecture)})
	}
	var id C.uint32_t
	C.swp_platform_set(s.e, &out[0], C.uint32_t(len(out)), &id)
	return id
}

// spreadSet: the preferences that create a decision-tree level (nodeset.go:59-82); others are skipped as the reference skips them
func (s *swpEngine) spreadSet(prefs []*api.PlacementPreference) C.uint32_t {
	var levels []C.swp_spread
	for _, pref := range prefs {
		sp := pref.GetSpread()
		if sp == nil {
			continue
		}
		if kind, id, ok := s.labelKey(sp.SpreadDescriptor); ok {
			levels = append(levels, C.swp_spread{kind: kind, key: id})
		}
	}
	if len(levels) == 0 {
		return 0
	}
	var id C.uint32_t
	C.swp_spread_set(s.e, &levels[0], C.uint32_t(len(levels)), &id)
	return id
}

// pluginSet: PluginFilter.SetTask (filter.go:119-131); what counts as a requirement follows Check (:133-177)
func (s *swpEngine) pluginSet(t *api.Task) (C.uint32_t, bool) {
	var req []C.uint32_t
	if c := t.Spec.GetContainer(); c != nil {
		for _, m := range c.Mounts {
			if m.Type == api.MountTypeVolume && m.VolumeOptions != nil && m.VolumeOptions.DriverConfig != nil {
				if name := m.VolumeOptions.DriverConfig.Name; name != "" && name != "local" {
					req = append(req, s.intern(C.SWP_SPACE_PLUGIN, "Volume\x00"+name))
				}
			}
		}
	}
	for _, na := range t.Networks {
		if na.Network != nil && na.Network.DriverState != nil && na.Network.DriverState.Name != "" {
			req = append(req, s.intern(C.SWP_SPACE_PLUGIN, "Network\x00"+na.Network.DriverState.Name))
		}
	}
	var log C.uint32_t
	if ld := t.Spec.LogDriver; ld != nil && ld.Name != "" && ld.Name != "none" {
		log = s.intern(C.SWP_SPACE_PLUGIN, "Log\x00"+ld.Name)
	}
	if len(req) == 0 && log == 0 {
		return 0, true
	}
	p := &log
	if len(req) > 0 {
		p = &req[0]
	}
	var id C.uint32_t
	C.swp_plugin_set(s.e, p, C.uint32_t(len(req)), log, &id)
	return id, true
}

// desc: Pipeline.SetTask → one swp_task_desc (every Filter.SetTask of pipeline.go:76-81); Scheduler::taskDesc.
// ok = false: the task stays on the reference's own path.
func (s *swpEngine) desc(t *api.Task) (d C.swp_task_desc, ok bool) {
	d.service = s.intern(C.SWP_SPACE_SERVICE, t.ServiceID)
	if r := t.Spec.Resources; r != nil && r.Reservations != nil { // ResourceFilter.SetTask, filter.go:61-74
		if d.generic_set, ok = s.genericSet(r.Reservations.Generic); !ok {
			return d, false
		}
		d.cpu, d.mem = C.int64_t(r.Reservations.NanoCPUs), C.int64_t(r.Reservations.MemoryBytes)
		if d.cpu != 0 || d.mem != 0 || d.generic_set != 0 {
			d.flags |= C.SWP_TASK_RES_ENABLED
		}
	}
	if t.DesiredState > api.TaskStateCompleted {
		d.flags |= 0x2 // the placement does not count toward ActiveTasksCount* (nodeinfo.go:148)
	}
	if pl := t.Spec.Placement; pl != nil {
		if cs, err := constraint.Parse(pl.Constraints); err == nil { // filter.go:218-232: an unparsable list disables the filter
			d.constraint_set = s.constraintSet(cs)
		}
		d.platform_set = s.platformSet(pl.Platforms)
		d.max_replicas = C.uint64_t(pl.MaxReplicas)
		d.spread_set = s.spreadSet(pl.Preferences)
	}
	if d.plugin_set, ok = s.pluginSet(t); !ok {
		return d, false
	}
	if d.port_set, ok = s.portSet(t); !ok {
		return d, false
	}
	if set, ok := s.mountSet(t); !ok { // VolumesFilter.SetTask, filter.go:392-422
		return d, false
	} else if set != 0 {
		d.flags |= C.uint32_t(set) << C.SWP_TASK_MOUNTS_SHIFT
	}
	if t.SpecVersion != nil {
		d.spec_version = C.uint64_t(t.SpecVersion.Index)
	}
	return d, true
}

// ---- CSI volumes (round 4): the engine judges VolumesFilter.Check and runs chooseTaskVolumes; volumeSet keeps its maps ----------

// upsertVolume: volumeSet.addOrUpdateVolume (volumes.go:62-82), from EventUpdateVolume (scheduler.go:200-213) and setupTasksList (:70-81)
func (s *swpEngine) upsertVolume(v *api.Volume) error {
	sv := C.swp_volume{group: s.intern(C.SWP_SPACE_VOLUME_GROUP, v.Spec.Group), driver: s.intern(C.SWP_SPACE_CSI, v.Spec.Driver.Name),
		scope: C.uint32_t(v.Spec.AccessMode.Scope), sharing: C.uint32_t(v.Spec.AccessMode.Sharing)}
	if v.Spec.Availability == api.VolumeAvailabilityActive {
		sv.active = 1
	}
	off := []C.uint32_t{0}
	var segs []C.swp_seg
	for _, top := range v.VolumeInfo.AccessibleTopology {
		keys := make([]string, 0, len(top.Segments))
		for k := range top.Segments {
			keys = append(keys, k)
		}
		sort.Strings(keys)
		for _, k := range keys {
			segs = append(segs, C.swp_seg{key: s.intern(C.SWP_SPACE_CSI, k), value: s.intern(C.SWP_SPACE_CSI, top.Segments[k])})
		}
		off = append(off, C.uint32_t(len(segs)))
	}
	sv.n_topologies = C.uint32_t(len(off) - 1)
	var none C.swp_seg
	p := &none
	if len(segs) > 0 {
		p = &segs[0]
	}
	idx := s.intern(C.SWP_SPACE_VOLUME, v.ID)
	for len(s.volumeID) <= int(idx) {
		s.volumeID = append(s.volumeID, "")
	}
	s.volumeID[idx] = v.ID
	if rc := C.swp_volume_upsert(s.e, idx, &sv, &off[0], p); rc != C.SWP_OK {
		return s.err("swp_volume_upsert", rc)
	}
	return nil
}

// Where the hooks go in volumes.go (three one-line additions, each behind `if vs.swp != nil`):
//   addOrUpdateVolume (:62-82)   vs.swp.upsertVolume(v)            — after the maps are updated
//   reserveVolume     (:156-167) vs.swp.pushVolumeUsage(volumeID, info)
//   releaseVolume     (:169-178) vs.swp.pushVolumeUsage(volumeID, info)
// and in scheduler.go: createOrUpdateNode / buildNodeSet call swp.upsert (which carries the node's CSIInfo), the nodeSet's remove
// calls swp.remove.

// pushVolumeUsage: after every volumeSet.reserveVolume / releaseVolume (volumes.go:156-187) — what checkVolume derives from info.tasks
func (s *swpEngine) pushVolumeUsage(volumeID string, info volumeInfo) {
	u := C.swp_volume_usage{pin: C.SWP_PIN_NONE}
	for _, usage := range info.tasks {
		u.n_tasks++
		if !usage.readOnly {
			u.n_writers++
		}
		idx, known := s.nodeIdx[usage.nodeID]
		switch {
		case !known:
			u.pin = C.SWP_PIN_MANY // a user on a node the nodeSet does not hold: no node of the set is that node
		case u.pin == C.SWP_PIN_NONE:
			u.pin = idx
		case u.pin != idx:
			u.pin = C.SWP_PIN_MANY
		}
	}
	C.swp_volume_set_usage(s.e, s.intern(C.SWP_SPACE_VOLUME, volumeID), &u)
}

// nodeCSI: Description.CSIInfo after swp_node_upsert (the first entry of a plugin is the one checkVolume takes, volumes.go:272-278)
func (s *swpEngine) nodeCSI(node C.uint32_t, infos []*api.NodeCSIInfo) {
	var cs []C.swp_csi
	var segs []C.swp_seg
	for _, ci := range infos {
		c := C.swp_csi{plugin: s.intern(C.SWP_SPACE_CSI, ci.PluginName), seg_off: C.uint32_t(len(segs))}
		if ci.AccessibleTopology != nil {
			c.has_topology = 1
			for k, v := range ci.AccessibleTopology.Segments {
				segs = append(segs, C.swp_seg{key: s.intern(C.SWP_SPACE_CSI, k), value: s.intern(C.SWP_SPACE_CSI, v)})
			}
		}
		c.n_seg = C.uint32_t(len(segs)) - c.seg_off
		cs = append(cs, c)
	}
	var noC C.swp_csi
	var noS C.swp_seg
	pc, ps := &noC, &noS
	if len(cs) > 0 {
		pc = &cs[0]
	}
	if len(segs) > 0 {
		ps = &segs[0]
	}
	C.swp_node_set_csi(s.e, node, pc, C.uint32_t(len(cs)), ps, C.uint32_t(len(segs)))
}

// mountSet: the task's MountTypeCluster mounts in spec order (VolumesFilter.SetTask); a name resolves through volumeSet.byName NOW
// (volumes.go:252). false: more mounts than the engine takes — the task stays on the Go path.
func (s *swpEngine) mountSet(t *api.Task) (C.uint32_t, bool) {
	c := t.Spec.GetContainer()
	if c == nil {
		return 0, true
	}
	var ms []C.swp_mount
	for _, m := range c.Mounts {
		if m.Type != api.MountTypeCluster {
			continue
		}
		mm := C.swp_mount{ref: C.SWP_NO_VOLUME}
		if group, ok := strings.CutPrefix(m.Source, "group:"); ok {
			mm.is_group, mm.ref = 1, s.intern(C.SWP_SPACE_VOLUME_GROUP, group)
		} else if id, ok := s.vs.byName[m.Source]; ok {
			mm.ref = s.intern(C.SWP_SPACE_VOLUME, id)
		}
		if m.ReadOnly {
			mm.read_only = 1
		}
		for _, other := range c.Mounts { // reserveTaskVolumes (volumes.go:148-151): the LAST mount with this (Source, Target) speaks
			if other.Source == m.Source && other.Target == m.Target {
				mm.reserve_read_only = 0
				if other.ReadOnly {
					mm.reserve_read_only = 1
				}
			}
		}
		ms = append(ms, mm)
	}
	if len(ms) == 0 {
		return 0, true
	}
	if len(ms) > C.SWP_MAX_MOUNTS {
		return 0, false
	}
	var id C.uint32_t
	if rc := C.swp_mount_set(s.e, &ms[0], C.uint32_t(len(ms)), &id); rc != C.SWP_OK {
		return 0, false
	}
	return id, true
}

// attachments: newT.Volumes for a task the batch placed (scheduler.go:862-872) from swp_batch_attachments' row; nil when a mount found no
// volume (the reference assigns the task without attachments). The caller then runs its own reserveTaskVolumes(&newT) (:874).
func (s *swpEngine) attachments(t *api.Task, row []C.uint32_t) []*api.VolumeAttachment {
	if len(row) == 0 || row[0] == C.SWP_NO_VOLUME {
		return nil
	}
	var out []*api.VolumeAttachment
	i := 0
	for _, m := range t.Spec.GetContainer().Mounts {
		if m.Type == api.MountTypeCluster {
			out = append(out, &api.VolumeAttachment{ID: s.volumeID[row[i]], Source: m.Source, Target: m.Target})
			i++
		}
	}
	return out
}

// commit: NodeInfo.addTask / removeTask from the event handlers (scheduler.go:254-366) and the rollback (:472-487)
func (s *swpEngine) commit(nodeID string, t *api.Task, add bool) {
	r := taskReservations(t.Spec)
	ports, _ := s.portSet(t)
	p := C.swp_placement{node: s.intern(C.SWP_SPACE_NODE_ID, nodeID), service: s.intern(C.SWP_SPACE_SERVICE, t.ServiceID),
		cpu: C.int64_t(r.NanoCPUs), mem: C.int64_t(r.MemoryBytes), port_set: ports}
	if t.DesiredState <= api.TaskStateCompleted {
		p.counted = 1
	}
	addFlag := C.int(0)
	if add {
		addFlag = 1
	}
	C.swp_commit(s.e, &p, 1, addFlag)
}

// pushFailures: the counts nodeLess reads (scheduler.go:706-735) for the services of the coming batch, at its `now`;
// a bucket the engine holds but the node no longer has (cleanupFailures, nodeinfo.go:163-183) goes back to 0.
func (sch *Scheduler) pushFailures(now time.Time, tasks []*api.Task) {
	s := sch.swp
	services := map[string]bool{}
	for _, t := range tasks {
		services[t.ServiceID] = true
	}
	cur := map[failureBucket]uint32{}
	for _, n := range sch.nodeSet.nodes {
		idx := s.intern(C.SWP_SPACE_NODE_ID, n.ID)
		for key := range n.recentFailures {
			if services[key.serviceID] {
				probe := &api.Task{ServiceID: key.serviceID, SpecVersion: &api.Version{Index: key.specVersion.Index}}
				cur[failureBucket{idx, key.serviceID, key.specVersion.Index}] = uint32(n.countRecentFailures(now, probe))
			}
		}
	}
	for b, c := range s.pushed {
		if _, still := cur[b]; services[b.service] && !still {
			if c != 0 {
				C.swp_node_set_failures(s.e, b.node, s.intern(C.SWP_SPACE_SERVICE, b.service), C.uint64_t(b.version), 0)
			}
			delete(s.pushed, b)
		}
	}
	for b, c := range cur {
		C.swp_node_set_failures(s.e, b.node, s.intern(C.SWP_SPACE_SERVICE, b.service), C.uint64_t(b.version), C.uint32_t(c))
		s.pushed[b] = c
	}
}

// explainFromHist: Pipeline.Explain (pipeline.go:84-103) from the engine's per-filter counters (index = position in the pipeline)
func explainFromHist(h []C.uint32_t) string {
	one := [...]string{"1 node not available for new tasks", "insufficient resources on 1 node", "missing plugin on 1 node",
		"scheduling constraints not satisfied on 1 node", "unsupported platform on 1 node", "host-mode port already in use on 1 node",
		"max replicas per node limit exceed", "cannot fulfill requested CSI volume mounts on 1 node"}
	many := [...]string{"%d nodes not available for new tasks", "insufficient resources on %d nodes", "missing plugin on %d nodes",
		"scheduling constraints not satisfied on %d nodes", "unsupported platform on %d nodes", "host-mode port already in use on %d nodes",
		"max replicas per node limit exceed", "cannot fulfill requested CSI volume mounts on %d nodes"}
	order := make([]int, len(h))
	for i := range order {
		order[i] = i
	}
	sort.SliceStable(order, func(a, b int) bool { return h[order[a]] > h[order[b]] }) // pipeline.go:90-93: most failures first, ties in pipeline order
	var parts []string
	for _, i := range order {
		switch n := h[i]; {
		case n == 1:
			parts = append(parts, one[i])
		case n > 1:
			parts = append(parts, strings.Replace(many[i], "%d", strconv.Itoa(int(n)), 1))
		}
	}
	return strings.Join(parts, "; ")
}

// ---------------------------------------------------------------------------------------------- tick()

// scheduleOneOffsSWP: the one-off branch of tick() (scheduler.go:467-469) becomes one batch. Returns the tasks the engine
// declined: they continue through scheduleTaskGroup as today.
func (sch *Scheduler) scheduleOneOffsSWP(ctx context.Context, tasks []*api.Task, decisions map[string]schedulingDecision) []*api.Task {
	descs := make([]C.swp_task_desc, 0, len(tasks))
	var kept, rest []*api.Task
	for _, t := range tasks {
		if d, ok := sch.swp.desc(t); ok {
			descs = append(descs, d)
			kept = append(kept, t)
		} else {
			rest = append(rest, t)
		}
	}
	if len(kept) == 0 {
		return rest
	}
	sch.pushFailures(time.Now(), kept)
	out := make([]C.int32_t, len(descs))
	hist := make([]C.uint32_t, len(descs)*C.SWP_NFILTERS)
	var mounted []C.uint32_t // the batch's tasks with cluster mounts: their attachments are read back
	for i := range descs {
		if descs[i].flags>>C.SWP_TASK_MOUNTS_SHIFT != 0 {
			mounted = append(mounted, C.uint32_t(i))
		}
	}
	att := make([]C.uint32_t, len(mounted)*C.SWP_MAX_MOUNTS)
	if len(mounted) == 0 {
		if rc := C.swp_schedule_batch(sch.swp.e, &descs[0], C.uint32_t(len(descs)), &out[0], &hist[0]); rc != C.SWP_OK {
			return tasks // the call was refused as a whole, nothing was applied: the Go scan takes this tick's one-off tasks
		}
	} else { // the same in three steps: the batch handle is needed for swp_batch_attachments (Scheduler::runOneOffs)
		var b *C.swp_batch
		if rc := C.swp_batch_prepare(sch.swp.e, &descs[0], C.uint32_t(len(descs)), &b); rc != C.SWP_OK {
			return tasks
		}
		rc := C.swp_batch_run(sch.swp.e, b)
		if rc == C.SWP_OK {
			rc = C.swp_batch_fetch(sch.swp.e, b, &out[0], &hist[0])
		}
		if rc == C.SWP_OK {
			rc = C.swp_batch_attachments(sch.swp.e, b, &mounted[0], C.uint32_t(len(mounted)), &att[0])
		}
		C.swp_batch_free(sch.swp.e, b)
		if rc != C.SWP_OK {
			return tasks
		}
	}
	m := 0
	for i, t := range kept {
		var vols []*api.VolumeAttachment
		if m < len(mounted) && int(mounted[m]) == i {
			vols = sch.swp.attachments(t, att[m*C.SWP_MAX_MOUNTS:(m+1)*C.SWP_MAX_MOUNTS])
			m++
		}
		if out[i] >= 0 {
			// newT.NodeID / Status ASSIGNED (scheduler.go:871-879), newT.Volumes = vols + reserveTaskVolumes(&newT) (:862-874); only
			// NodeInfo.Tasks changes: the engine already did the arithmetic
			sch.assign(ctx, t, sch.swp.idxNode[out[i]], vols, decisions)
		} else {
			sch.noSuitableNodeWith(ctx, t, explainFromHist(hist[i*C.SWP_NFILTERS:(i+1)*C.SWP_NFILTERS]), decisions)
		}
	}
	return rest
}

// scheduleOneOffsStreamedSWP: the same batch through swp_schedule_batch_streamed — the placements arrive range by range while later
// rounds still run, and every range goes straight to the store, applySchedulingDecisions' way (scheduler.go:490-643: one store.Batch
// transaction per 200 decisions), instead of after the last round, the copy of all placements and their replay into the node mirror.
// For batches without cluster mounts (their attachments are read after swp_batch_fetch). The C side needs a trampoline, because cgo
// passes no Go closure as a C function pointer:
//
//	//export swpPrefixSink
//	func swpPrefixSink(ctx unsafe.Pointer, first, count C.uint32_t, nodes *C.int32_t) C.int {
//		return cgo.Handle(uintptr(ctx)).Value().(func(first int, nodes []C.int32_t) C.int)(int(first), unsafe.Slice(nodes, int(count)))
//	}
//
// and in the preamble: `extern int swpPrefixSink(void*, uint32_t, uint32_t, int32_t*);` (cast to swp_prefix_sink at the call).
//
// What is delivered is final (include/swp.h): a task in a range will not move, and the engine's node mirror already holds it. What is NOT
// known before the call returns is whether the batch as a whole succeeds: on any return but SWP_OK every delivered range is void. So the
// sink may build and commit store transactions only if the caller can take them back (rollbackSWP's path for a failed transaction), or
// — as here — it stages the decisions per range (assign() fills `decisions`, which tick() hands to applySchedulingDecisions) and starts
// the store batch on the ranges it has, committing nothing before the return code is known; a non-zero return from the sink (ctx
// cancelled) cancels the batch: SWP_ECANCELLED, nothing applied, the Go scan takes the tick.
func (sch *Scheduler) scheduleOneOffsStreamedSWP(ctx context.Context, kept []*api.Task, descs []C.swp_task_desc, decisions map[string]schedulingDecision) bool {
	out := make([]C.int32_t, len(descs))
	hist := make([]C.uint32_t, len(descs)*C.SWP_NFILTERS)
	staged := 0 // tasks [0, staged) have their decision
	sink := func(first int, nodes []C.int32_t) C.int {
		if ctx.Err() != nil {
			return 1
		}
		for i, n := range nodes {
			if n >= 0 { // (a task without a node needs its Explain row: after the call)
				sch.assign(ctx, kept[first+i], sch.swp.idxNode[n], nil, decisions)
			}
		}
		staged = first + len(nodes)
		return 0
	}
	h := cgo.NewHandle(sink)
	defer h.Delete()
	rc := C.swp_schedule_batch_streamed(sch.swp.e, &descs[0], C.uint32_t(len(descs)), &out[0], &hist[0],
		C.swp_prefix_sink(C.swpPrefixSink), unsafe.Pointer(uintptr(h)), 200) // min_tasks: a store transaction's worth
	if rc != C.SWP_OK {
		// every delivered range is void: the decisions staged for them go, with the NodeInfo.Tasks entries assign() made. NOT through
		// rollbackSWP: the engine's side is already as before the call, a swp_commit(remove) would take the tasks out twice
		for _, t := range kept[:staged] {
			if d, ok := decisions[t.ID]; ok {
				if ni, err := sch.nodeSet.nodeInfo(d.new.NodeID); err == nil {
					delete(ni.Tasks, d.new.ID)
					sch.nodeSet.updateNode(ni)
				}
				delete(decisions, t.ID)
			}
		}
		return false
	}
	for i, t := range kept {
		if out[i] < 0 {
			sch.noSuitableNodeWith(ctx, t, explainFromHist(hist[i*C.SWP_NFILTERS:(i+1)*C.SWP_NFILTERS]), decisions)
		}
	}
	return true
}

// scheduleGroupsSWP: the grouped branch (scheduler.go:456-461) — every (ServiceID, SpecVersion) group in one call
func (sch *Scheduler) scheduleGroupsSWP(ctx context.Context, groups []map[string]*api.Task, decisions map[string]schedulingDecision) {
	var descs []C.swp_task_desc
	var sizes []C.uint32_t
	var order [][]*api.Task // canonical (enqueue) order inside a group
	var all []*api.Task
	for _, tg := range groups {
		ts := sortedByEnqueue(tg)
		d, ok := sch.swp.desc(ts[0]) // all tasks of a group are identical for the filters (scheduler.go:696-702)
		if !ok {
			sch.scheduleTaskGroup(ctx, tg, decisions)
			continue
		}
		descs, sizes, order = append(descs, d), append(sizes, C.uint32_t(len(ts))), append(order, ts)
		all = append(all, ts...)
	}
	if len(descs) == 0 {
		return
	}
	sch.pushFailures(time.Now(), all)
	out := make([]C.int32_t, len(all))
	hist := make([]C.uint32_t, len(descs)*C.SWP_NFILTERS)
	anyMounts := false
	for i := range descs {
		anyMounts = anyMounts || descs[i].flags>>C.SWP_TASK_MOUNTS_SHIFT != 0
	}
	var att []C.uint32_t
	var rc C.int
	if anyMounts { // out_att[i * SWP_MAX_MOUNTS + m]: the volume chosen for mount m of the call's i-th task
		att = make([]C.uint32_t, len(all)*C.SWP_MAX_MOUNTS)
		rc = C.swp_schedule_groups_volumes(sch.swp.e, &descs[0], &sizes[0], C.uint32_t(len(descs)), &out[0], &hist[0], &att[0])
	} else {
		rc = C.swp_schedule_groups(sch.swp.e, &descs[0], &sizes[0], C.uint32_t(len(descs)), &out[0], &hist[0])
	}
	if rc != C.SWP_OK {
		for _, ts := range order { // a group beyond the engine's capacity (SWP_ERANGE): nothing was applied, the Go path takes them
			tg := map[string]*api.Task{}
			for _, t := range ts {
				tg[t.ID] = t
			}
			sch.scheduleTaskGroup(ctx, tg, decisions)
		}
		return
	}
	i := 0
	for g, ts := range order {
		for _, t := range ts {
			if out[i] >= 0 {
				var vols []*api.VolumeAttachment
				if anyMounts {
					vols = sch.swp.attachments(t, att[i*C.SWP_MAX_MOUNTS:(i+1)*C.SWP_MAX_MOUNTS])
				}
				sch.assign(ctx, t, sch.swp.idxNode[out[i]], vols, decisions)
			} else {
				sch.noSuitableNodeWith(ctx, t, explainFromHist(hist[g*C.SWP_NFILTERS:(g+1)*C.SWP_NFILTERS]), decisions)
			}
			i++
		}
	}
}

// scheduleGroupsStreamedSWP: the grouped tick through swp_schedule_groups_streamed, for a call without cluster mounts (descs, sizes,
// order, all as scheduleGroupsSWP builds them): the tick is ONE launch that decides group after group, and the kernel itself hands out
// what is decided — a range always ends at a group boundary and holds at least min_tasks tasks (200: a store transaction's worth), so
// applySchedulingDecisions (scheduler.go:490-643) can start on the first groups while the later ones are still decided. The trampoline
// is scheduleOneOffsStreamedSWP's (swpPrefixSink), and so is the rule: nothing delivered is valid unless the call returns SWP_OK — the
// sink stages decisions (assign) and commits nothing; on any other code the engine's side is already as before the call and the staged
// decisions go. A group's Explain counters (and a call's attachments) are complete only when the call returns: tasks without a node are
// handled behind it.
func (sch *Scheduler) scheduleGroupsStreamedSWP(ctx context.Context, descs []C.swp_task_desc, sizes []C.uint32_t, order [][]*api.Task, all []*api.Task,
	decisions map[string]schedulingDecision) bool {
	out := make([]C.int32_t, len(all))
	hist := make([]C.uint32_t, len(descs)*C.SWP_NFILTERS)
	staged := 0 // tasks [0, staged) of `all` have their decision
	sink := func(first int, nodes []C.int32_t) C.int {
		if ctx.Err() != nil {
			return 1 // SWP_ECANCELLED: the kernel ends at the next group it publishes, the engine rolls the ranges back
		}
		for i, n := range nodes {
			if n >= 0 {
				sch.assign(ctx, all[first+i], sch.swp.idxNode[n], nil, decisions)
			}
		}
		staged = first + len(nodes)
		return 0
	}
	h := cgo.NewHandle(sink)
	defer h.Delete()
	rc := C.swp_schedule_groups_streamed(sch.swp.e, &descs[0], &sizes[0], C.uint32_t(len(descs)), &out[0], &hist[0], nil,
		C.swp_prefix_sink(C.swpPrefixSink), unsafe.Pointer(uintptr(h)), 200)
	if rc != C.SWP_OK {
		for _, t := range all[:staged] { // every delivered range is void (not through rollbackSWP: the engine has taken them out itself)
			if d, ok := decisions[t.ID]; ok {
				if ni, err := sch.nodeSet.nodeInfo(d.new.NodeID); err == nil {
					delete(ni.Tasks, d.new.ID)
					sch.nodeSet.updateNode(ni)
				}
				delete(decisions, t.ID)
			}
		}
		return false // the caller falls back to scheduleGroupsSWP or the Go path
	}
	i := 0
	for g, ts := range order {
		for _, t := range ts {
			if out[i] < 0 {
				sch.noSuitableNodeWith(ctx, t, explainFromHist(hist[g*C.SWP_NFILTERS:(g+1)*C.SWP_NFILTERS]), decisions)
			}
			i++
		}
	}
	return true
}

// rollbackSWP: the failed half of applySchedulingDecisions (scheduler.go:472-487): the reference already restores allTasks,
// calls nodeInfo.removeTask(decision.new) and enqueues decision.old; the engine side of removeTask is one swp_commit(remove).
func (sch *Scheduler) rollbackSWP(failed []schedulingDecision) {
	for _, d := range failed {
		if d.new.NodeID != "" {
			sch.swp.commit(d.new.NodeID, d.new, false)
		}
	}
}

// sortedByEnqueue, assign and noSuitableNodeWith are three-line wrappers around code that exists in scheduler.go
// (the task order of a group, the body of scheduleNTasksOnNodes' inner loop :857-897 without the numeric addTask — newT.Volumes = the
// attachments passed in, then s.volumes.reserveTaskVolumes(&newT) exactly as :862-874 — and noSuitableNode :928-971 with the
// explanation passed in instead of s.pipeline.Explain()).

// Several GPUs: the scheduler holds a shard SET (newSwpShardSet) in sch.swp and the two functions above run unchanged — one-off
// batches become sharded batches (the rounds on the devices, include/swp.h "node-range shards"; nodeset.go:57-120 is the scan they
// distribute), task groups run on the set's union engine, tasks with cluster mounts included. A manager that runs one PROCESS per GPU
// calls swp_rccl_unique_id / swp_rccl_init once and swp_shard_run_rank per batch instead (bench.py --gpus N is that deployment).

// ---------------------------------------------------------------------------------------------- constraint enforcer
// The enforcer (manager/orchestrator/constraintenforcer) shares the scheduler's engine: rejectNoncompliantTasksSWP in INTEGRATION.md
// builds the records of its sweep and calls enforceSweep. Nodes whose tasks hold AssignedGenericResources go through the same call:
// the loop's last third (constraint_enforcer.go:186-200) runs on the device too. Scheduler::enforce

// enforceRes: a generic resource list as swp_enforce_res entries, LIST ORDER kept. A named value is an id handed out per sweep (`names`):
// equal strings <=> equal ids. An entry with an empty oneof is left out (its Kind() is "" and nothing ever matches it).
func (s *swpEngine) enforceRes(dst []C.swp_enforce_res, rs []*api.GenericResource, names map[string]C.int64_t) []C.swp_enforce_res {
	for _, r := range rs {
		if n := r.GetNamedResourceSpec(); n != nil {
			id, ok := names[n.Value]
			if !ok {
				id = C.int64_t(len(names))
				names[n.Value] = id
			}
			dst = append(dst, C.swp_enforce_res{kind: s.intern(C.SWP_SPACE_GENERIC_KIND, n.Kind), named: 1, value: id})
		} else if d := r.GetDiscreteResourceSpec(); d != nil {
			dst = append(dst, C.swp_enforce_res{kind: s.intern(C.SWP_SPACE_GENERIC_KIND, d.Kind), named: 0, value: C.int64_t(d.Value)})
		}
	}
	return dst
}

// enforceSweep: one swp_enforce_generic call. nodeOff / taskOff: where each node's available.Generic and each task's
// AssignedGenericResources lie in nodeRes / taskRes (one offset per record and one behind the last). reject[i] != 0: task i would be set
// to REJECTED. An error leaves the caller on the reference's rejectNoncompliantTasks, node by node.
func (s *swpEngine) enforceSweep(nodes []C.swp_enforce_node, tasks []C.swp_enforce_task, nodeOff []C.uint32_t, nodeRes []C.swp_enforce_res,
	taskOff []C.uint32_t, taskRes []C.swp_enforce_res) ([]C.uint8_t, error) {
	reject := make([]C.uint8_t, len(tasks))
	if len(nodes) == 0 || len(tasks) == 0 {
		return reject, nil
	}
	var nr, tr *C.swp_enforce_res // (an empty array: the offsets name no entry of it)
	if len(nodeRes) > 0 {
		nr = &nodeRes[0]
	}
	if len(taskRes) > 0 {
		tr = &taskRes[0]
	}
	if rc := C.swp_enforce_generic(s.e, &nodes[0], C.uint32_t(len(nodes)), &tasks[0], C.uint32_t(len(tasks)), &nodeOff[0], nr, &taskOff[0], tr, &reject[0]); rc != C.SWP_OK {
		return nil, s.err("swp_enforce_generic", rc)
	}
	return reject, nil
}
