// SPVBuffer.cpp -- host/device mirrored sliding-DFT container (reference: src/flan/SPV/SPVBuffer.cpp).
#include "flan/SPVBuffer.h"

#include <iostream>
#include <utility>

#include "device_block.h"

namespace flan {

SPVBuffer::SPVBuffer() : format(), buffer() {}
SPVBuffer::SPVBuffer( const Format & f ) : format( f ), buffer() {}

SPVBuffer SPVBuffer::adopt_device( const Format & f, std::shared_ptr<detail::DeviceBlock> block )
	{
	SPVBuffer out( f );
	out.dev = std::move( block );
	out.host_valid = false;
	return out;
	}

SPVBuffer SPVBuffer::copy() const
	{
	SPVBuffer out( format );
	out.buffer = get_buffer();
	return out;
	}

bool SPVBuffer::is_null() const
	{
	return get_sample_rate() <= 0 || count() == 0;
	}

void SPVBuffer::clear_buffer()
	{
	auto held = lock.hold();
	buffer.assign( count(), MF{ 0.0f, 0.0f } );
	host_valid = true;
	dev.reset();
	}

void SPVBuffer::materialize_locked() const
	{
	if( !host_valid )
		{
		if( buffer.capacity() < count() )
			{
			buffer.reserve( count() );
			detail::touch_pages( buffer.data(), sizeof( MF ) * count() );
			}
		buffer.resize( count() );
		if( dev && count() && !detail::download_to_host( buffer.data(), dev->ptr, sizeof( MF ) * count() ) )
			std::cerr << "flan: download of SPV failed: " << flanhip_last_error() << std::endl;
		host_valid = true;
		}
	else if( buffer.size() != count() ) buffer.assign( count(), MF{ 0.0f, 0.0f } );      // a buffer made from a Format: zeros, now
	}

const std::vector<MF> & SPVBuffer::get_buffer() const
	{
	auto held = lock.hold();
	materialize_locked();
	return buffer;
	}

std::vector<MF> & SPVBuffer::get_buffer()
	{
	auto held = lock.hold();
	materialize_locked();
	dev.reset();                       // the caller may write: the device copy is stale
	return buffer;
	}

MF SPVBuffer::get_MF( Channel c, Frame f, Bin b ) const { return get_buffer()[get_buffer_pos( c, f, b )]; }
MF & SPVBuffer::get_MF( Channel c, Frame f, Bin b ) { return get_buffer()[get_buffer_pos( c, f, b )]; }

std::shared_ptr<detail::DeviceBlock> SPVBuffer::device_block() const
	{
	auto held = lock.hold();
	if( !dev )
		{
		if( count() == 0 ) return nullptr;
		materialize_locked();
		auto block = detail::DeviceBlock::allocate( sizeof( MF ) * count() );
		if( !block ) return nullptr;
		if( !detail::upload_from_host( block->ptr, buffer.data(), sizeof( MF ) * count() ) )
			{
			std::cerr << "flan: upload of SPV failed: " << flanhip_last_error() << std::endl;
			return nullptr;
			}
		dev = std::move( block );
		}
	return dev;
	}

const MF * SPVBuffer::device_data() const
	{
	const auto block = device_block();
	return block ? static_cast<const MF*>( block->ptr ) : nullptr;
	}

} // namespace flan
