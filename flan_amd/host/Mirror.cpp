// Mirror.cpp -- the transfers behind flan::detail::Mirror<T> (flan/mirror.h), instantiated for the two element types.
#include "flan/mirror.h"

#include <iostream>

#include "device_block.h"
#include "flan/defines.h"

namespace flan { namespace detail {

template<typename T>
void Mirror<T>::materialize( size_t count ) const
	{
	if( !host_valid )
		{
		if( buffer.capacity() < count )                  // fresh memory: let every worker fault its share of the pages in, not this thread alone
			{
			buffer.reserve( count );
			touch_pages( buffer.data(), sizeof( T ) * count );
			}
		buffer.resize( count );
		if( dev && count && !download_to_host( buffer.data(), dev->ptr, sizeof( T ) * count ) )
			std::cerr << "flan: download of " << noun << " failed: " << flanhip_last_error() << std::endl;
		host_valid = true;
		}
	else if( lazy_zeros && buffer.size() != count ) buffer.assign( count, T{} );      // a buffer made from a Format: zeros, now
	}

template<typename T>
void Mirror<T>::clear( size_t count, std::shared_ptr<DeviceBlock> * derived )
	{
	auto held = hold();
	buffer.assign( count, T{} );
	host_valid = true;
	dev.reset();
	if( derived ) derived->reset();
	}

template<typename T>
const std::vector<T> & Mirror<T>::host( size_t count ) const
	{
	auto held = hold();
	materialize( count );              // once host_valid is set no const method touches the vector again
	return buffer;
	}

template<typename T>
std::vector<T> & Mirror<T>::host( size_t count, std::shared_ptr<DeviceBlock> * derived )
	{
	auto held = hold();
	materialize( count );
	dev.reset();                       // the host copy is the truth from here on, and anything derived from the old data is stale
	if( derived ) derived->reset();
	return buffer;
	}

template<typename T>
std::shared_ptr<DeviceBlock> Mirror<T>::device_block( size_t count ) const
	{
	auto held = hold();
	if( !dev )
		{
		if( count == 0 ) return nullptr;
		materialize( count );
		if( buffer.size() < count ) return nullptr;      // (a moved-from owner: its format outlives its data)
		auto block = DeviceBlock::allocate( sizeof( T ) * count );
		if( !block ) return nullptr;
		if( !upload_from_host( block->ptr, buffer.data(), sizeof( T ) * count ) )
			{
			std::cerr << "flan: upload of " << noun << " failed: " << flanhip_last_error() << std::endl;
			return nullptr;
			}
		dev = std::move( block );
		}
	return dev;
	}

template<typename T>
const T * Mirror<T>::device_data( size_t count ) const
	{
	const auto block = device_block( count );
	return block ? static_cast<const T*>( block->ptr ) : nullptr;
	}

template class Mirror<float>;
template class Mirror<MF>;

} }
